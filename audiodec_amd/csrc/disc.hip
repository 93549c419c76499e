// HiFi-GAN discriminator (models/vocoder/modules/discriminator.py:27-449) and the adversarial / feature-matching loss sums
// (losses/adversarial_loss.py, losses/feat_match_loss.py), exact f32: the forward, and the backward to the input (the gradient
// of the generator-side GAN losses with respect to y_hat through every conv, pooling and padding step; the weights are
// constants).  The backward is in gather form: every dx element is written exactly once by one thread or one accumulator,
// nothing is added atomically, so the gradient is bitwise reproducible.
//
// Every conv of both sub-discriminators is one shape: a non-causal, zero-padded, strided, grouped conv along H of an
// (N, C_in, H, P) tensor whose element (h, j) sits at h*P + j -- P = 1 for the scale discriminator's Conv1d, P = period for the
// period discriminator's (k, 1) Conv2d.  Output (h', j) lands at h'*P + j of (N, C_out, H', P), the reference's own layout, so
// there is no transpose and no padded copy: the padding is predicated loads.
//   GEMM form, per group g:  Y[m][n] = bias[m] + sum_kk W[m][kk] X[kk][n],  m < C_out/g,  kk = ci*k + t < (C_in/g)*k,
//                            n = (item, h', j) over every output position;  X[kk][n] = x[item][g*C_in/g + ci][h'*s - pad + t][j]
//   backward:  dx[i][g cin_g + ci][h][j] = sum over co of group g and taps t with (h + pad - t) % stride == 0,
//                            0 <= ho = (h + pad - t) / stride < H'  of W[co][ci][t] dz[i][co][ho][j],   dz = cg_dz(dy, y)
//                            (y the layer's saved post-activation output: y > 0 exactly where its pre-activation is, for slope >= 0).
//
//   disc_gemm_kernel:        the forward GEMM through conv_gemm_f32.h's core (W pre-transposed at load to [g][kk][m]); DiscSrc is
//                            the addressing above.  Groups are the grid's z dimension.
//   disc_direct_kernel:      one thread per output (or 8 threads splitting C_in/g, summed in a fixed order), for the C_in = 1 first
//                            layers and the C_out = 1 output layers, where a GEMM tile would be mostly padding.
//   disc_gemm_grad_kernel:   the backward sum as a GEMM through the same core:  M = C_in/g (rows of dx), N = input positions,
//                            K = (co, tap) pairs.  A strided layer is split by PHASE r = (h + pad) % stride: only the taps
//                            t = r, r + stride, ... can reach such an h, so the columns are enumerated per phase, blockIdx.z
//                            runs over (group, phase) and the K loop of a grid slice runs over cout_g * taps(r) pairs only --
//                            no structural zero is multiplied.  W is re-packed at load to [g][phase][kk = co * taps(r) + tt][m].
//                            A phase without taps (kernel < stride) has K = 0 and writes zeros; so do rows the forward never
//                            read (every ho out of range).  The activation mask is applied where a tap is staged (DiscGradSrc::tap).
//   disc_direct_grad_kernel: one thread per dx element (or 8 threads splitting C_out/g, summed in a fixed order), for the
//                            C_in/g = 1 first layers -- whose dx IS the waveform gradient -- and the C_out/g = 1 output layers.
//   disc_prep_kernel:        right-side reflect padding (the period discriminator's F.pad(x, (0, n_pad), "reflect")) and
//                            AvgPool1d with count_include_pad (the scale discriminator's pooling between scales).
//   disc_prep_grad_kernel:   the backward of both, as gathers.
//   disc_loss_kernel:        sum over a tensor of (x-1)^2, x^2, |a-b|, x, min(x-1, 0) or min(-x-1, 0) (f32 term, f64 sum) through
//                            per-workgroup f64 partials and a fixed-order finalize launch (reduce_f64.h): bitwise reproducible.
//   disc_loss_grad_kernel:   g[i] = c * term'(a[i], b[i]) for those six terms, c = (float)(coef * upstream[0]) with the upstream
//                            gradient read on the device.
#include "conv_gemm_f32.h"
#include "reduce_f64.h"

namespace adk {

constexpr int DISC_PREP_REFLECT = 0, DISC_PREP_AVGPOOL = 1;
constexpr int DISC_LOSS_MSE_ONE = 0, DISC_LOSS_SQ = 1, DISC_LOSS_L1 = 2, DISC_LOSS_SUM = 3, DISC_LOSS_HINGE_REAL = 4,
              DISC_LOSS_HINGE_FAKE = 5;
constexpr int DISC_LOSS_MAX_WG = 1024;
constexpr int DISC_DIRECT_SPLIT = 8;

// One layer as both directions see it; filled by disc_geometry.
struct DiscGeom {
    int n_items, c_in, h_in, period, c_out, groups, ksz, stride, pad, h_out, act;
    int cin_g, cout_g;
    float slope;
    long long hp_in, hp_out;                        // h_in * period, h_out * period: positions per channel
};

struct DiscConv : CgForwardPtrs, DiscGeom {         // x [n_items][c_in][h_in][period] -> y [n_items][c_out][h_out][period]
    int kg;                                         // cin_g * ksz: GEMM K
    long long n_cols;                               // n_items * hp_out: GEMM N
};
struct DiscGrad : CgBackwardPtrs, DiscGeom {};      // dy, y of y's shape -> dx of x's

// What conv_gemm_f32 needs of a DiscConv: group g = blockIdx.z; tap kk = ci*k + t of a column is a division along H.
struct DiscSrc {
    const DiscConv& c;
    const int g = blockIdx.z;
    long long xbase = 0;
    int hb = -0x40000000;                           // an invalid column fails the bounds test
    __device__ int k_extent() const { return c.kg; }
    __device__ int m_extent() const { return c.cout_g; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w + (size_t)g * c.kg * c.cout_g; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.hp_out;
            const long long rem = col - item * c.hp_out;
            const int ho = (int)(rem / c.period), j = (int)(rem - (long long)ho * c.period);
            xbase = ((item * c.c_in + (long long)g * c.cin_g) * c.h_in) * c.period + j;
            hb = ho * c.stride - c.pad;
        }
    }
    __device__ float tap(int kk) const {
        const int ci = kk / c.ksz, h = hb + (kk - ci * c.ksz);
        const bool ok = kk < c.kg && (unsigned)h < (unsigned)c.h_in;
        return ok ? c.x[xbase + ((long long)ci * c.h_in + h) * c.period] : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.hp_out, rem = n - item * c.hp_out;
        return c.y + (item * c.c_out + (long long)g * c.cout_g) * c.hp_out + rem;
    }
    __device__ long long out_stride() const { return c.hp_out; }
    __device__ int bias_index(int m) const { return g * c.cout_g + m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void disc_gemm_kernel(DiscConv c) {
    DiscSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, c.bias, c.act, c.slope);
}

// One output per x-thread; blockDim.y threads split the group's input channels and are summed in y order.
__global__ __launch_bounds__(CG_THREADS) void disc_direct_kernel(DiscConv c) {
    __shared__ float part[CG_THREADS];
    const int split = blockDim.y;
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = c.n_cols * c.c_out;
    float s = 0.f;
    long long item = 0, rem = 0;
    int co = 0;
    if (o < total) {
        rem = o % c.hp_out;
        const long long t = o / c.hp_out;
        co = (int)(t % c.c_out);
        item = t / c.c_out;
        const int ho = (int)(rem / c.period), j = (int)(rem - (long long)ho * c.period);
        const int g = co / c.cout_g;
        const int per = (c.cin_g + split - 1) / split;
        const int ci0 = threadIdx.y * per, ci1 = min(c.cin_g, ci0 + per);
        const float* __restrict__ wr = c.w + (size_t)co * c.kg;
        const float* __restrict__ xb = c.x + ((item * c.c_in + (long long)g * c.cin_g) * c.h_in) * c.period + j;
        const int hb = ho * c.stride - c.pad;
        for (int ci = ci0; ci < ci1; ++ci) {
            const float* xc = xb + (long long)ci * c.h_in * c.period;
            for (int t2 = 0; t2 < c.ksz; ++t2) {
                const int h = hb + t2;
                if ((unsigned)h < (unsigned)c.h_in) s = fmaf(wr[ci * c.ksz + t2], xc[(long long)h * c.period], s);
            }
        }
    }
    if (split > 1) {
        part[threadIdx.y * blockDim.x + threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.y != 0) return;
        for (int q = 1; q < split; ++q) s += part[q * blockDim.x + threadIdx.x];
    }
    if (o < total) {
        const float bias = c.bias ? c.bias[co] : 0.f;
        c.y[(item * c.c_out + co) * c.hp_out + rem] = cg_act(s + bias, c.act, c.slope);
    }
}

// What conv_gemm_f32 needs of a DiscGrad: blockIdx.z = g * stride + r.  Column (item, q, j) of phase r is input row
// h = h0 + q stride, h0 the first row with (h + pad) % stride == r; K index kk = co * nt + tt is tap t = r + tt stride of output
// channel co, which reads output row ho = (h + pad) / stride - tt.
struct DiscGradSrc {
    const DiscGrad& c;
    const int g = blockIdx.z / c.stride;
    const int r = blockIdx.z - g * c.stride;
    const int nt = phase_taps(c.ksz, c.stride, r);
    const int h0 = phase_first(c.pad, c.stride, r);
    const int nh = phase_count(c.h_in, c.stride, h0);
    const long long per_item = (long long)nh * c.period;
    const long long ncols = (long long)c.n_items * per_item;
    const int taps_before = phase_taps_before(c.ksz, c.stride, r);
    long long ybase = 0;
    int u = -0x40000000;                            // an invalid column fails the bounds test
    __device__ int k_extent() const { return c.cout_g * nt; }
    __device__ int m_extent() const { return c.cin_g; }
    __device__ long long n_cols() const { return ncols; }
    __device__ const float* weights() const {
        return c.w + ((size_t)g * c.ksz + taps_before) * c.cout_g * c.cin_g;
    }
    __device__ void column(long long col) {
        if (col < ncols) {
            const long long item = col / per_item, rem = col - item * per_item;
            const int q = (int)(rem / c.period), j = (int)(rem - (long long)q * c.period);
            ybase = (item * c.c_out + (long long)g * c.cout_g) * c.hp_out + j;
            u = (h0 + q * c.stride + c.pad) / c.stride;
        }
    }
    __device__ float tap(int kk) const {
        const int co = kk / max(nt, 1), ho = u - (kk - co * nt);
        const bool ok = kk < c.cout_g * nt && (unsigned)ho < (unsigned)c.h_out;
        return ok ? cg_dz(c.dy, c.y, c.act, c.slope, ybase + ((long long)co * c.h_out + ho) * c.period) : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / per_item, rem = n - item * per_item;
        const long long q = rem / c.period, j = rem - q * c.period;
        return c.dx + (item * c.c_in + (long long)g * c.cin_g) * c.hp_in + ((long long)h0 + q * c.stride) * c.period + j;
    }
    __device__ long long out_stride() const { return c.hp_in; }
    __device__ int bias_index(int m) const { return m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void disc_gemm_grad_kernel(DiscGrad c) {
    DiscGradSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, nullptr, CG_ACT_NONE, 0.f);
}

// One dx element per x-thread; blockDim.y threads split the group's output channels and are summed in y order.
// w is the reference's layout [c_out][c_in/groups][kernel].
__global__ __launch_bounds__(CG_THREADS) void disc_direct_grad_kernel(DiscGrad c) {
    __shared__ float part[CG_THREADS];
    const int split = blockDim.y;
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)c.n_items * c.c_in * c.hp_in;
    float s = 0.f;
    if (o < total) {
        const long long rem = o % c.hp_in, t = o / c.hp_in;
        const int cf = (int)(t % c.c_in);
        const long long item = t / c.c_in;
        const int h = (int)(rem / c.period), j = (int)(rem - (long long)h * c.period);
        const int g = cf / c.cin_g, ci = cf - g * c.cin_g;
        const int r = (h + c.pad) % c.stride, u = (h + c.pad) / c.stride;
        const int per = (c.cout_g + split - 1) / split;
        const int co0 = threadIdx.y * per, co1 = min(c.cout_g, co0 + per);
        for (int co = co0; co < co1; ++co) {
            const int cof = g * c.cout_g + co;
            const float* __restrict__ wr = c.w + ((size_t)cof * c.cin_g + ci) * c.ksz;
            const long long base = (item * c.c_out + cof) * c.hp_out + j;
            int ho = u;
            for (int t2 = r; t2 < c.ksz && ho >= 0; t2 += c.stride, --ho)
                if (ho < c.h_out) s = fmaf(wr[t2], cg_dz(c.dy, c.y, c.act, c.slope, base + (long long)ho * c.period), s);
        }
    }
    if (split > 1) {
        part[threadIdx.y * blockDim.x + threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.y != 0) return;
        for (int q = 1; q < split; ++q) s += part[q * blockDim.x + threadIdx.x];
    }
    if (o < total) c.dx[o] = s;
}

// op REFLECT: y [rows][n_in + a] = x, then x[2 (n_in - 1) - t] for t >= n_in  (a < n_in).
// op AVGPOOL: y [rows][(n_in + 2c - a) / b + 1],  y[i] = sum_{q < a} x[i b - c + q] (zero outside) / a.
__global__ __launch_bounds__(CG_THREADS) void disc_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int n_in,
                                                               int n_out, int op, int a, int b, int c) {
    const long long total = (long long)rows * n_out;
    for (long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x; o < total; o += (long long)gridDim.x * CG_THREADS) {
        const long long r = o / n_out;
        const int i = (int)(o - r * n_out);
        const float* xr = x + r * n_in;
        float v;
        if (op == DISC_PREP_REFLECT) {
            v = xr[i < n_in ? i : 2 * (n_in - 1) - i];
        } else {
            float s = 0.f;
            const int t0 = i * b - c;
            for (int q = 0; q < a; ++q) {
                const int t = t0 + q;
                if ((unsigned)t < (unsigned)n_in) s += xr[t];
            }
            v = s / (float)a;
        }
        y[o] = v;
    }
}

// op REFLECT:  dx[i] = dy[i] + dy[2 (n_in - 1) - i] where that mirror index lies in [n_in, n_in + a).
// op AVGPOOL:  dx[t] = (sum of dy[i] over the windows i that contain t) / a.
__global__ __launch_bounds__(CG_THREADS) void disc_prep_grad_kernel(const float* __restrict__ dy, float* __restrict__ dx, int rows,
                                                                    int n_in, int n_out, int op, int a, int b, int c) {
    const long long total = (long long)rows * n_in;
    for (long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x; o < total; o += (long long)gridDim.x * CG_THREADS) {
        const long long row = o / n_in;
        const int t = (int)(o - row * n_in);
        const float* gr = dy + row * n_out;
        float v;
        if (op == DISC_PREP_REFLECT) {
            const long long m = 2LL * (n_in - 1) - t;
            v = gr[t];
            if (m >= n_in && m < n_out) v += gr[m];
        } else {
            const long long lo = (long long)t + c - a + 1;
            const int i0 = lo <= 0 ? 0 : (int)((lo + b - 1) / b);
            const int i1 = (int)min((long long)n_out - 1, ((long long)t + c) / b);
            float s = 0.f;
            for (int i = i0; i <= i1; ++i) s += gr[i];
            v = s / (float)a;
        }
        dx[o] = v;
    }
}

static int disc_loss_workgroups(long long n) {
    return capped_workgroups((n + 4LL * CG_THREADS - 1) / (4LL * CG_THREADS), DISC_LOSS_MAX_WG);
}

template <int KIND>
__device__ __forceinline__ double disc_term(const float* __restrict__ a, const float* __restrict__ b, long long i) {
    const float v = a[i];
    if constexpr (KIND == DISC_LOSS_MSE_ONE) { const float d = v - 1.f; return (double)(d * d); }
    if constexpr (KIND == DISC_LOSS_SQ) return (double)(v * v);
    if constexpr (KIND == DISC_LOSS_L1) return (double)fabsf(v - b[i]);
    if constexpr (KIND == DISC_LOSS_SUM) return (double)v;
    if constexpr (KIND == DISC_LOSS_HINGE_REAL) return (double)fminf(v - 1.f, 0.f);
    return (double)fminf(-v - 1.f, 0.f);
}

template <int KIND>
__global__ __launch_bounds__(CG_THREADS) void disc_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                               double* __restrict__ partial) {
    double acc[1] = {0.0};
    for (long long i = (long long)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CG_THREADS)
        acc[0] += disc_term<KIND>(a, b, i);
    workgroup_partials<1, CG_THREADS / 64>(acc, partial);
}

__global__ __launch_bounds__(CG_THREADS) void disc_loss_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    long long n, int kind, double coef,
                                                                    const float* __restrict__ upstream, float* __restrict__ g) {
    const float c = (float)(coef * (double)upstream[0]);
    for (long long i = (long long)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CG_THREADS) {
        const float v = a[i];
        float d;
        switch (kind) {
            case DISC_LOSS_MSE_ONE: d = 2.f * (v - 1.f); break;
            case DISC_LOSS_SQ: d = 2.f * v; break;
            case DISC_LOSS_L1: {
                const float e = v - b[i];
                d = e != e ? e : (float)((e > 0.f) - (e < 0.f));
                break;
            }
            case DISC_LOSS_SUM: d = 1.f; break;
            case DISC_LOSS_HINGE_REAL: d = v < 1.f ? 1.f : 0.f; break;
            default: d = v > -1.f ? -1.f : 0.f; break;
        }
        g[i] = c * d;
    }
}

template <int WM, int WN, int TM, int TN>
static void launch_gemm(const DiscConv& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((c.n_cols + BN - 1) / BN), (unsigned)((c.cout_g + BM - 1) / BM), (unsigned)c.groups);
    hipLaunchKernelGGL((disc_gemm_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), 0, s, c);
}

// The backward GEMM's grid is sized for the phase with most columns, the one with h0 = 0.
static long long disc_grad_max_cols(const DiscGrad& c) {
    return (long long)c.n_items * ((c.h_in + c.stride - 1) / c.stride) * c.period;
}

template <int WM, int WN, int TM, int TN>
static void launch_gemm_grad(const DiscGrad& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((disc_grad_max_cols(c) + BN - 1) / BN), (unsigned)((c.cin_g + BM - 1) / BM),
                    (unsigned)(c.groups * c.stride));
    hipLaunchKernelGGL((disc_gemm_grad_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), 0, s, c);
}

// The checks adk_disc_conv and adk_disc_conv_grad both make of a layer, in their order, and its geometry.  `masked`: the
// backward, which takes the LeakyReLU mask from the layer's output and so needs slope >= 0.  The direction's own size limits and
// its pointers are the caller's to check next.
static int disc_geometry(const std::string& f, int n_items, int c_in, int h_in, int period, int c_out, int groups, int kernel,
                         int stride, int pad, int act, float slope, int impl, bool masked, DiscGeom& g) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || period <= 0 || c_out <= 0 || groups <= 0 || kernel <= 0 || stride <= 0 || pad < 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, h_in, period, c_out, groups, kernel, stride > 0, pad >= 0");
    if (c_in % groups || c_out % groups) return fail(ADK_ERR_ARG, f + ": groups must divide c_in and c_out");
    int rc = cg_check_act_impl(f, act, slope, impl, masked);
    if (rc != ADK_OK) return rc;
    const long long span = (long long)h_in + 2LL * pad - kernel;
    if (span < 0) return fail(ADK_ERR_ARG, f + ": kernel longer than the padded input");
    const long long h_out = span / stride + 1;
    g.n_items = n_items; g.c_in = c_in; g.h_in = h_in; g.period = period; g.c_out = c_out; g.groups = groups;
    g.ksz = kernel; g.stride = stride; g.pad = pad; g.h_out = (int)h_out; g.act = act; g.slope = slope;
    g.cin_g = c_in / groups; g.cout_g = c_out / groups;
    g.hp_in = (long long)h_in * period; g.hp_out = h_out * period;
    return ADK_OK;
}

// The checks adk_disc_prep and adk_disc_prep_grad both make of an op on rows of n_in, and the length n_out of its output rows.
static int disc_prep_geometry(const std::string& f, int rows, int n_in, int op, int a, int b, int c, long long& n_out) {
    if (rows < 0 || n_in <= 0) return fail(ADK_ERR_ARG, f + ": need rows >= 0, n_in > 0");
    if (op == DISC_PREP_REFLECT) {
        if (a < 0 || a >= n_in) return fail(ADK_ERR_ARG, f + ": reflect padding needs 0 <= n_pad < n_in");
        n_out = (long long)n_in + a;
    } else if (op == DISC_PREP_AVGPOOL) {
        if (a <= 0 || b <= 0 || c < 0 || 2 * c > a) return fail(ADK_ERR_ARG, f + ": avgpool needs kernel, stride > 0, 0 <= pad <= kernel/2");
        if ((long long)n_in + 2LL * c < a) return fail(ADK_ERR_ARG, f + ": avgpool kernel longer than the padded input");
        n_out = ((long long)n_in + 2LL * c - a) / b + 1;
    } else {
        return fail(ADK_ERR_ARG, f + ": op must be 0 (reflect) or 1 (avgpool)");
    }
    if (n_out >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": row too long");
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_disc_conv(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in,
                             int32_t h_in, int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride,
                             int32_t pad, int32_t act, float slope, int32_t impl, void* stream) {
    const std::string f = "adk_disc_conv";
    DiscConv c;
    int rc = disc_geometry(f, n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad, act, slope, impl, false, c);
    if (rc != ADK_OK) return rc;
    if ((long long)c.cin_g * kernel >= (1LL << 30) || c.hp_out >= (1LL << 40)) return fail(ADK_ERR_ARG, f + ": layer too large");
    rc = check_pointers(f, "x/w/bias/y", n_items > 0 && (!x || !w || !y), {x, w, bias, y});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.x = x; c.w = w; c.bias = bias; c.y = y;
    c.kg = c.cin_g * kernel;
    c.n_cols = (long long)n_items * c.hp_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    if (impl == CG_IMPL_DIRECT) {
        const int split = c.cin_g >= 64 ? DISC_DIRECT_SPLIT : 1;
        const int bx = CG_THREADS / split;
        const long long total = c.n_cols * c_out;
        const long long nb = (total + bx - 1) / bx;
        if (nb >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": layer too large for the direct kernel");
        hipLaunchKernelGGL(disc_direct_kernel, dim3((unsigned)nb), dim3(bx, split), 0, s, c);
    } else {
        if ((c.n_cols + 31) / 32 >= (1LL << 31) || groups > 65535)
            return fail(ADK_ERR_ARG, f + ": layer too large for the gemm kernel");
        if (c.cout_g >= 128) launch_gemm<2, 2, 2, 2>(c, s);            // 128 x 128
        else if (c.cout_g >= 64) launch_gemm<2, 2, 1, 2>(c, s);        // 64 x 128
        else launch_gemm<1, 4, 1, 1>(c, s);                            // 32 x 128
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_conv_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in,
                                  int32_t h_in, int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride,
                                  int32_t pad, int32_t act, float slope, int32_t impl, void* stream) {
    const std::string f = "adk_disc_conv_grad";
    DiscGrad c;
    int rc = disc_geometry(f, n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad, act, slope, impl, true, c);
    if (rc != ADK_OK) return rc;
    if ((long long)c.cout_g * kernel >= (1LL << 30) || c.hp_in >= (1LL << 40) || (long long)h_in + pad >= (1LL << 30) ||
        (long long)pad + stride >= (1LL << 30))
        return fail(ADK_ERR_ARG, f + ": layer too large");
    rc = check_pointers(f, "dy/y/w/dx", n_items > 0 && (!dy || !w || !dx || (act == CG_ACT_LEAKY && !y)), {dy, y, w, dx});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.dy = dy; c.y = y; c.w = w; c.dx = dx;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    if (impl == CG_IMPL_DIRECT) {
        const int split = c.cout_g >= 64 ? DISC_DIRECT_SPLIT : 1;
        const int bx = CG_THREADS / split;
        const long long total = (long long)n_items * c_in * c.hp_in;
        const long long nb = (total + bx - 1) / bx;
        if (nb >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": layer too large for the direct kernel");
        hipLaunchKernelGGL(disc_direct_grad_kernel, dim3((unsigned)nb), dim3(bx, split), 0, s, c);
    } else {
        if ((disc_grad_max_cols(c) + 31) / 32 >= (1LL << 31) || (long long)groups * stride > 65535)
            return fail(ADK_ERR_ARG, f + ": layer too large for the gemm kernel");
        if (c.cin_g >= 128) launch_gemm_grad<2, 2, 2, 2>(c, s);           // 128 x 128
        else if (c.cin_g >= 64) launch_gemm_grad<2, 2, 1, 2>(c, s);       // 64 x 128
        else launch_gemm_grad<1, 4, 1, 1>(c, s);                          // 32 x 128
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_prep(const float* x, float* y, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c,
                             void* stream) {
    const std::string f = "adk_disc_prep";
    long long n_out;
    int rc = disc_prep_geometry(f, rows, n_in, op, a, b, c, n_out);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "x/y", rows > 0 && (!x || !y), {x, y});
    if (rc != ADK_OK) return rc;
    if (rows == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    const long long total = (long long)rows * n_out;
    const int nb = (int)std::min<long long>((total + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_prep_kernel, dim3(nb), dim3(CG_THREADS), 0, s, x, y, rows, n_in, (int)n_out, op, a, b, c);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_prep_grad(const float* dy, float* dx, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c,
                                  void* stream) {
    const std::string f = "adk_disc_prep_grad";
    long long n_out;
    int rc = disc_prep_geometry(f, rows, n_in, op, a, b, c, n_out);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/dx", rows > 0 && (!dy || !dx), {dy, dx});
    if (rc != ADK_OK) return rc;
    if (rows == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    const long long total = (long long)rows * n_in;
    const int nb = (int)std::min<long long>((total + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_prep_grad_kernel, dim3(nb), dim3(CG_THREADS), 0, s, dy, dx, rows, n_in, (int)n_out, op, a, b, c);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int64_t adk_disc_loss_workspace_bytes(int64_t n) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_disc_loss_workspace_bytes: need n >= 0");
    if (n == 0) return 0;
    return (int64_t)disc_loss_workgroups(n) * (int64_t)sizeof(double);
}

extern "C" int adk_disc_loss(const float* a, const float* b, int64_t n, int32_t kind, double* sum, int64_t* count, void* workspace,
                             float* loss, void* stream) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_disc_loss: need n >= 0");
    if (kind < DISC_LOSS_MSE_ONE || kind > DISC_LOSS_HINGE_FAKE) return fail(ADK_ERR_ARG, "adk_disc_loss: kind must be 0..5");
    const int rc = check_accumulators("adk_disc_loss", sum, count, workspace, n > 0, loss, nullptr);
    if (rc != ADK_OK) return rc;
    if (n > 0 && (!a || (kind == DISC_LOSS_L1 && !b))) return fail(ADK_ERR_ARG, "adk_disc_loss: null pointer");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_loss: a/b must be 4-byte aligned");
    if (n == 0 && !loss) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sum));
    const int n_wg = n > 0 ? disc_loss_workgroups(n) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n > 0) {
        switch (kind) {
            case DISC_LOSS_MSE_ONE: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_MSE_ONE>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
            case DISC_LOSS_SQ: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_SQ>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
            case DISC_LOSS_L1: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_L1>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
            case DISC_LOSS_SUM: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_SUM>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
            case DISC_LOSS_HINGE_REAL: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_HINGE_REAL>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
            default: hipLaunchKernelGGL(disc_loss_kernel<DISC_LOSS_HINGE_FAKE>, dim3(n_wg), dim3(CG_THREADS), 0, s, a, b, n, partial); break;
        }
        ADK_HIP_CHECK(hipGetLastError());
    }
    launch_distance_finalize<1>(partial, n_wg, (long long)n, sum, count, nullptr, loss, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_loss_grad(const float* a, const float* b, int64_t n, int32_t kind, double coef, const float* upstream,
                                  float* grad, void* stream) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_disc_loss_grad: need n >= 0");
    if (kind < DISC_LOSS_MSE_ONE || kind > DISC_LOSS_HINGE_FAKE) return fail(ADK_ERR_ARG, "adk_disc_loss_grad: kind must be 0..5");
    const int rc = check_pointers("adk_disc_loss_grad", "a/b/upstream/grad",
                                     n > 0 && (!a || !upstream || !grad || (kind == DISC_LOSS_L1 && !b)), {a, b, upstream, grad});
    if (rc != ADK_OK) return rc;
    if (n == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad));
    const int nb = (int)std::min<long long>((n + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_loss_grad_kernel, dim3(nb), dim3(CG_THREADS), 0, s, a, b, (long long)n, kind, coef, upstream, grad);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
