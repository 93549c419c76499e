// HiFi-GAN discriminator forward (models/vocoder/modules/discriminator.py:27-449) and the adversarial / feature-matching loss sums
// (losses/adversarial_loss.py, losses/feat_match_loss.py), exact f32.
//
// Every conv of both sub-discriminators is one shape: a non-causal, zero-padded, strided, grouped conv along H of an
// (N, C_in, H, P) tensor whose element (h, j) sits at h*P + j -- P = 1 for the scale discriminator's Conv1d, P = period for the
// period discriminator's (k, 1) Conv2d.  Output (h', j) lands at h'*P + j of (N, C_out, H', P), the reference's own layout, so
// there is no transpose and no padded copy: the padding is predicated loads.
//   GEMM form, per group g:  Y[m][n] = bias[m] + sum_kk W[m][kk] X[kk][n],  m < C_out/g,  kk = ci*k + t < (C_in/g)*k,
//                            n = (item, h', j) over every output position;  X[kk][n] = x[item][g*C_in/g + ci][h'*s - pad + t][j]
//   disc_gemm_kernel:   that GEMM through conv_gemm_f32.h's core (W pre-transposed at load to [g][kk][m]); DiscSrc is the
//                       addressing above.  Groups are the grid's z dimension.
//   disc_direct_kernel: one thread per output (or 8 threads splitting C_in/g, summed in a fixed order), for the C_in = 1 first
//                       layers and the C_out = 1 output layers, where a GEMM tile would be mostly padding.
//   disc_prep_kernel:   right-side reflect padding (the period discriminator's F.pad(x, (0, n_pad), "reflect")) and
//                       AvgPool1d with count_include_pad (the scale discriminator's pooling between scales).
//   disc_loss_kernel:   sum over a tensor of (x-1)^2, x^2, |a-b|, x, min(x-1, 0) or min(-x-1, 0) (f32 term, f64 sum) through
//                       per-workgroup f64 partials and a fixed-order finalize launch (reduce_f64.h): bitwise reproducible.
#include "conv_gemm_f32.h"
#include "reduce_f64.h"

namespace adk {

constexpr int DISC_PREP_REFLECT = 0, DISC_PREP_AVGPOOL = 1;
constexpr int DISC_LOSS_MSE_ONE = 0, DISC_LOSS_SQ = 1, DISC_LOSS_L1 = 2, DISC_LOSS_SUM = 3, DISC_LOSS_HINGE_REAL = 4,
              DISC_LOSS_HINGE_FAKE = 5;
constexpr int DISC_LOSS_MAX_WG = 1024;
constexpr int DISC_DIRECT_SPLIT = 8;

struct DiscConv {
    const float* x;
    const float* w;
    const float* bias;                              // [c_out] or null
    float* y;
    int n_items, c_in, h_in, period, c_out, groups, ksz, stride, pad, h_out, act;
    int cin_g, cout_g, kg;                          // kg = cin_g * ksz
    float slope;
    long long hp_out;                               // h_out * period: output positions per channel
    long long n_cols;                               // n_items * hp_out: GEMM N
};

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

template <int WM, int WN, int TM, int TN>
static void launch_gemm(const DiscConv& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((c.n_cols + BN - 1) / BN), (unsigned)((c.cout_g + BM - 1) / BM), (unsigned)c.groups);
    hipLaunchKernelGGL((disc_gemm_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), 0, s, c);
}

}  // namespace adk

using namespace adk;

extern "C" int adk_disc_conv(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in,
                             int32_t h_in, int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride,
                             int32_t pad, int32_t act, float slope, int32_t impl, void* stream) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || period <= 0 || c_out <= 0 || groups <= 0 || kernel <= 0 || stride <= 0 || pad < 0)
        return fail(ADK_ERR_ARG, "adk_disc_conv: need n_items >= 0, c_in, h_in, period, c_out, groups, kernel, stride > 0, pad >= 0");
    if (c_in % groups || c_out % groups) return fail(ADK_ERR_ARG, "adk_disc_conv: groups must divide c_in and c_out");
    if (act != CG_ACT_NONE && act != CG_ACT_LEAKY) return fail(ADK_ERR_ARG, "adk_disc_conv: act must be 0 (none) or 2 (leaky)");
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, "adk_disc_conv: impl must be 1 (direct) or 2 (gemm)");
    const long long span = (long long)h_in + 2LL * pad - kernel;
    if (span < 0) return fail(ADK_ERR_ARG, "adk_disc_conv: kernel longer than the padded input");
    const long long h_out = span / stride + 1;
    if ((long long)(c_in / groups) * kernel >= (1LL << 30) || h_out * period >= (1LL << 40))
        return fail(ADK_ERR_ARG, "adk_disc_conv: layer too large");
    if (n_items > 0 && (!x || !w || !y)) return fail(ADK_ERR_ARG, "adk_disc_conv: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) |
         reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_conv: x/w/bias/y must be 4-byte aligned");
    if (n_items == 0) return ADK_OK;
    DiscConv c;
    c.x = x; c.w = w; c.bias = bias; c.y = y;
    c.n_items = n_items; c.c_in = c_in; c.h_in = h_in; c.period = period; c.c_out = c_out; c.groups = groups;
    c.ksz = kernel; c.stride = stride; c.pad = pad; c.h_out = (int)h_out; c.act = act; c.slope = slope;
    c.cin_g = c_in / groups; c.cout_g = c_out / groups; c.kg = c.cin_g * kernel;
    c.hp_out = h_out * period;
    c.n_cols = (long long)n_items * c.hp_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    if (impl == CG_IMPL_DIRECT) {
        const int split = c.cin_g >= 64 ? DISC_DIRECT_SPLIT : 1;
        const int bx = CG_THREADS / split;
        const long long total = c.n_cols * c_out;
        const long long nb = (total + bx - 1) / bx;
        if (nb >= (1LL << 31)) return fail(ADK_ERR_ARG, "adk_disc_conv: layer too large for the direct kernel");
        hipLaunchKernelGGL(disc_direct_kernel, dim3((unsigned)nb), dim3(bx, split), 0, s, c);
    } else {
        if ((c.n_cols + 31) / 32 >= (1LL << 31) || groups > 65535)
            return fail(ADK_ERR_ARG, "adk_disc_conv: layer too large for the gemm kernel");
        if (c.cout_g >= 128) launch_gemm<2, 2, 2, 2>(c, s);            // 128 x 128
        else if (c.cout_g >= 64) launch_gemm<2, 2, 1, 2>(c, s);        // 64 x 128
        else launch_gemm<1, 4, 1, 1>(c, s);                            // 32 x 128
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_prep(const float* x, float* y, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c,
                             void* stream) {
    if (rows < 0 || n_in <= 0) return fail(ADK_ERR_ARG, "adk_disc_prep: need rows >= 0, n_in > 0");
    long long n_out;
    if (op == DISC_PREP_REFLECT) {
        if (a < 0 || a >= n_in) return fail(ADK_ERR_ARG, "adk_disc_prep: reflect padding needs 0 <= n_pad < n_in");
        n_out = (long long)n_in + a;
    } else if (op == DISC_PREP_AVGPOOL) {
        if (a <= 0 || b <= 0 || c < 0 || 2 * c > a) return fail(ADK_ERR_ARG, "adk_disc_prep: avgpool needs kernel, stride > 0, 0 <= pad <= kernel/2");
        if ((long long)n_in + 2LL * c < a) return fail(ADK_ERR_ARG, "adk_disc_prep: avgpool kernel longer than the padded input");
        n_out = ((long long)n_in + 2LL * c - a) / b + 1;
    } else {
        return fail(ADK_ERR_ARG, "adk_disc_prep: op must be 0 (reflect) or 1 (avgpool)");
    }
    if (n_out >= (1LL << 31)) return fail(ADK_ERR_ARG, "adk_disc_prep: row too long");
    if (rows > 0 && (!x || !y)) return fail(ADK_ERR_ARG, "adk_disc_prep: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_prep: x/y must be 4-byte aligned");
    if (rows == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    const long long total = (long long)rows * n_out;
    const int nb = (int)std::min<long long>((total + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_prep_kernel, dim3(nb), dim3(CG_THREADS), 0, s, x, y, rows, n_in, (int)n_out, op, a, b, c);
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
