// HiFi-GAN discriminator backward to its input (the gradient of the generator-side GAN losses with respect to y_hat through
// every conv, pooling and padding step of disc.hip; the weights are constants), exact f32, in gather form: every dx element is
// written exactly once by one thread or one accumulator, nothing is added atomically, so the gradient is bitwise reproducible.
//
//   dx[i][g cin_g + ci][h][j] = sum over co of group g and taps t with (h + pad - t) % stride == 0, 0 <= ho = (h + pad - t) / stride < H'
//                               of W[co][ci][t] dz[i][co][ho][j],   dz = dy * (act ? (y > 0 ? 1 : slope) : 1)
//   (y the layer's saved post-activation output: y > 0 exactly where its pre-activation is, for slope >= 0).
//
//   disc_gemm_grad_kernel:   that sum as a GEMM through conv_gemm_f32.h's core:  M = C_in/g (rows of dx), N = input positions,
//                            K = (co, tap) pairs.  A strided layer is split by PHASE r = (h + pad) % stride: only the taps
//                            t = r, r + stride, ... can reach such an h, so the columns are enumerated per phase, blockIdx.z
//                            runs over (group, phase) and the K loop of a grid slice runs over cout_g * taps(r) pairs only --
//                            no structural zero is multiplied.  W is re-packed at load to [g][phase][kk = co * taps(r) + tt][m].
//                            A phase without taps (kernel < stride) has K = 0 and writes zeros; so do rows the forward never
//                            read (every ho out of range).  The activation mask is applied where a tap is staged (DiscGradSrc::tap).
//   disc_direct_grad_kernel: one thread per dx element (or 8 threads splitting C_out/g, summed in a fixed order), for the
//                            C_in/g = 1 first layers -- whose dx IS the waveform gradient -- and the C_out/g = 1 output layers.
//   disc_prep_grad_kernel:   the backward of right-side reflect padding and of AvgPool1d(count_include_pad), as gathers.
//   disc_loss_grad_kernel:   g[i] = c * term'(a[i], b[i]) for the six terms of adk_disc_loss, c = (float)(coef * upstream[0]) with
//                            the upstream gradient read on the device.
#include "conv_gemm_f32.h"

namespace adk {

constexpr int DG_PREP_REFLECT = 0, DG_PREP_AVGPOOL = 1;
constexpr int DG_LOSS_MSE_ONE = 0, DG_LOSS_SQ = 1, DG_LOSS_L1 = 2, DG_LOSS_SUM = 3, DG_LOSS_HINGE_REAL = 4, DG_LOSS_HINGE_FAKE = 5;
constexpr int DG_DIRECT_SPLIT = 8;

struct DiscGrad {
    const float* dy;                                // [n_items][c_out][h_out][period]
    const float* y;                                 // same shape: the forward's output (read when act is leaky)
    const float* w;
    float* dx;                                      // [n_items][c_in][h_in][period]
    int n_items, c_in, h_in, period, c_out, groups, ksz, stride, pad, h_out, act;
    int cin_g, cout_g;
    float slope;
    long long hp_in, hp_out;                        // h_in * period, h_out * period
};

__device__ __forceinline__ float disc_dz(const DiscGrad& c, long long idx) {
    const float v = c.dy[idx];
    return (c.act == CG_ACT_LEAKY && !(c.y[idx] > 0.f)) ? v * c.slope : v;
}

// What conv_gemm_f32 needs of a DiscGrad: blockIdx.z = g * stride + r.  Column (item, q, j) of phase r is input row
// h = h0 + q stride, h0 the first row with (h + pad) % stride == r; K index kk = co * nt + tt is tap t = r + tt stride of output
// channel co, which reads output row ho = (h + pad) / stride - tt.
struct DiscGradSrc {
    const DiscGrad& c;
    const int g = blockIdx.z / c.stride;
    const int r = blockIdx.z - g * c.stride;
    const int nt = r < c.ksz ? (c.ksz - r + c.stride - 1) / c.stride : 0;          // taps of this phase
    const int h0 = ((r - c.pad) % c.stride + c.stride) % c.stride;
    const int nh = h0 < c.h_in ? (c.h_in - h0 + c.stride - 1) / c.stride : 0;       // rows of this phase
    const long long per_item = (long long)nh * c.period;
    const long long ncols = (long long)c.n_items * per_item;
    const int taps_before = (c.ksz / c.stride) * r + min(c.ksz % c.stride, r);      // taps of the phases < r
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
        return ok ? disc_dz(c, ybase + ((long long)co * c.h_out + ho) * c.period) : 0.f;
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
                if (ho < c.h_out) s = fmaf(wr[t2], disc_dz(c, base + (long long)ho * c.period), s);
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

// op REFLECT (forward y [rows][n_in + a] = x, then x[2 (n_in - 1) - t] for t >= n_in):
//   dx[i] = dy[i] + dy[2 (n_in - 1) - i] where that mirror index lies in [n_in, n_in + a).
// op AVGPOOL (forward y[i] = sum_{q < a} x[i b - c + q] / a):  dx[t] = (sum of dy[i] over the windows i that contain t) / a.
__global__ __launch_bounds__(CG_THREADS) void disc_prep_grad_kernel(const float* __restrict__ dy, float* __restrict__ dx, int rows,
                                                                    int n_in, int n_out, int op, int a, int b, int c) {
    const long long total = (long long)rows * n_in;
    for (long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x; o < total; o += (long long)gridDim.x * CG_THREADS) {
        const long long row = o / n_in;
        const int t = (int)(o - row * n_in);
        const float* gr = dy + row * n_out;
        float v;
        if (op == DG_PREP_REFLECT) {
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

__global__ __launch_bounds__(CG_THREADS) void disc_loss_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    long long n, int kind, double coef,
                                                                    const float* __restrict__ upstream, float* __restrict__ g) {
    const float c = (float)(coef * (double)upstream[0]);
    for (long long i = (long long)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CG_THREADS) {
        const float v = a[i];
        float d;
        switch (kind) {
            case DG_LOSS_MSE_ONE: d = 2.f * (v - 1.f); break;
            case DG_LOSS_SQ: d = 2.f * v; break;
            case DG_LOSS_L1: {
                const float e = v - b[i];
                d = e != e ? e : (float)((e > 0.f) - (e < 0.f));
                break;
            }
            case DG_LOSS_SUM: d = 1.f; break;
            case DG_LOSS_HINGE_REAL: d = v < 1.f ? 1.f : 0.f; break;
            default: d = v > -1.f ? -1.f : 0.f; break;
        }
        g[i] = c * d;
    }
}

template <int WM, int WN, int TM, int TN>
static void launch_gemm_grad(const DiscGrad& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const long long max_cols = (long long)c.n_items * ((c.h_in + c.stride - 1) / c.stride) * c.period;   // the phase with h0 = 0
    const dim3 grid((unsigned)((max_cols + BN - 1) / BN), (unsigned)((c.cin_g + BM - 1) / BM), (unsigned)(c.groups * c.stride));
    hipLaunchKernelGGL((disc_gemm_grad_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), 0, s, c);
}

}  // namespace adk

using namespace adk;

extern "C" int adk_disc_conv_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in,
                                  int32_t h_in, int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride,
                                  int32_t pad, int32_t act, float slope, int32_t impl, void* stream) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || period <= 0 || c_out <= 0 || groups <= 0 || kernel <= 0 || stride <= 0 || pad < 0)
        return fail(ADK_ERR_ARG, "adk_disc_conv_grad: need n_items >= 0, c_in, h_in, period, c_out, groups, kernel, stride > 0, pad >= 0");
    if (c_in % groups || c_out % groups) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: groups must divide c_in and c_out");
    if (act != CG_ACT_NONE && act != CG_ACT_LEAKY) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: act must be 0 (none) or 2 (leaky)");
    if (act == CG_ACT_LEAKY && !(slope >= 0.f))
        return fail(ADK_ERR_ARG, "adk_disc_conv_grad: the mask is taken from the output, which needs slope >= 0");
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: impl must be 1 (direct) or 2 (gemm)");
    const long long span = (long long)h_in + 2LL * pad - kernel;
    if (span < 0) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: kernel longer than the padded input");
    const long long h_out = span / stride + 1;
    if ((long long)(c_out / groups) * kernel >= (1LL << 30) || (long long)h_in * period >= (1LL << 40) ||
        (long long)h_in + pad >= (1LL << 30) || (long long)pad + stride >= (1LL << 30))
        return fail(ADK_ERR_ARG, "adk_disc_conv_grad: layer too large");
    if (n_items > 0 && (!dy || !w || !dx || (act == CG_ACT_LEAKY && !y))) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: null pointer");
    if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w) |
         reinterpret_cast<uintptr_t>(dx)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_conv_grad: dy/y/w/dx must be 4-byte aligned");
    if (n_items == 0) return ADK_OK;
    DiscGrad c;
    c.dy = dy; c.y = y; c.w = w; c.dx = dx;
    c.n_items = n_items; c.c_in = c_in; c.h_in = h_in; c.period = period; c.c_out = c_out; c.groups = groups;
    c.ksz = kernel; c.stride = stride; c.pad = pad; c.h_out = (int)h_out; c.act = act; c.slope = slope;
    c.cin_g = c_in / groups; c.cout_g = c_out / groups;
    c.hp_in = (long long)h_in * period; c.hp_out = h_out * period;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    if (impl == CG_IMPL_DIRECT) {
        const int split = c.cout_g >= 64 ? DG_DIRECT_SPLIT : 1;
        const int bx = CG_THREADS / split;
        const long long total = (long long)n_items * c_in * c.hp_in;
        const long long nb = (total + bx - 1) / bx;
        if (nb >= (1LL << 31)) return fail(ADK_ERR_ARG, "adk_disc_conv_grad: layer too large for the direct kernel");
        hipLaunchKernelGGL(disc_direct_grad_kernel, dim3((unsigned)nb), dim3(bx, split), 0, s, c);
    } else {
        const long long max_cols = (long long)n_items * ((h_in + stride - 1) / stride) * period;
        if ((max_cols + 31) / 32 >= (1LL << 31) || (long long)groups * stride > 65535)
            return fail(ADK_ERR_ARG, "adk_disc_conv_grad: layer too large for the gemm kernel");
        if (c.cin_g >= 128) launch_gemm_grad<2, 2, 2, 2>(c, s);           // 128 x 128
        else if (c.cin_g >= 64) launch_gemm_grad<2, 2, 1, 2>(c, s);       // 64 x 128
        else launch_gemm_grad<1, 4, 1, 1>(c, s);                          // 32 x 128
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_prep_grad(const float* dy, float* dx, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c,
                                  void* stream) {
    if (rows < 0 || n_in <= 0) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: need rows >= 0, n_in > 0");
    long long n_out;
    if (op == DG_PREP_REFLECT) {
        if (a < 0 || a >= n_in) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: reflect padding needs 0 <= n_pad < n_in");
        n_out = (long long)n_in + a;
    } else if (op == DG_PREP_AVGPOOL) {
        if (a <= 0 || b <= 0 || c < 0 || 2 * c > a) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: avgpool needs kernel, stride > 0, 0 <= pad <= kernel/2");
        if ((long long)n_in + 2LL * c < a) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: avgpool kernel longer than the padded input");
        n_out = ((long long)n_in + 2LL * c - a) / b + 1;
    } else {
        return fail(ADK_ERR_ARG, "adk_disc_prep_grad: op must be 0 (reflect) or 1 (avgpool)");
    }
    if (n_out >= (1LL << 31)) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: row too long");
    if (rows > 0 && (!dy || !dx)) return fail(ADK_ERR_ARG, "adk_disc_prep_grad: null pointer");
    if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_prep_grad: dy/dx must be 4-byte aligned");
    if (rows == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    const long long total = (long long)rows * n_in;
    const int nb = (int)std::min<long long>((total + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_prep_grad_kernel, dim3(nb), dim3(CG_THREADS), 0, s, dy, dx, rows, n_in, (int)n_out, op, a, b, c);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_disc_loss_grad(const float* a, const float* b, int64_t n, int32_t kind, double coef, const float* upstream,
                                  float* grad, void* stream) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_disc_loss_grad: need n >= 0");
    if (kind < DG_LOSS_MSE_ONE || kind > DG_LOSS_HINGE_FAKE) return fail(ADK_ERR_ARG, "adk_disc_loss_grad: kind must be 0..5");
    if (n > 0 && (!a || !upstream || !grad || (kind == DG_LOSS_L1 && !b))) return fail(ADK_ERR_ARG, "adk_disc_loss_grad: null pointer");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(upstream) |
         reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail(ADK_ERR_ARG, "adk_disc_loss_grad: a/b/upstream/grad must be 4-byte aligned");
    if (n == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad));
    const int nb = (int)std::min<long long>((n + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(disc_loss_grad_kernel, dim3(nb), dim3(CG_THREADS), 0, s, a, b, (long long)n, kind, coef, upstream, grad);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
