// The symmetric decoder (models/autoencoder/modules/decoder.py:25-138) as a frozen, differentiable function of its input: a
// non-streaming forward on (B, C, T) tensors that writes every layer's output to memory, and the backward to the input with the
// weights held constant.  Exact f32 through conv_gemm_f32.h's core; every output element is written exactly once by one thread
// or one accumulator, nothing is added atomically, so forward and gradient are bitwise reproducible.  The streaming programs'
// chain kernels keep their activations in LDS and never write the pre-activations a backward needs, so they are not used here.
//
// a is a conv's INPUT activation (conv_gemm_f32.h's in_act), none, ELU(alpha) or LeakyReLU(alpha):
//   ELU    a(x) = x > 0 ? x : alpha expm1_neg(x)  (the inference kernels' ELU for alpha = 1), a'(x) = x > 0 ? 1 : alpha (expm1_neg(x) + 1)
//   Leaky  a(x) = x > 0 ? x : alpha x,                                                        a'(x) = x > 0 ? 1 : alpha
// The adk_dec_* entry points (the symmetric decoder) take none or ELU and one group; the adk_voc_* ones (the HiFi-GAN vocoder)
// take all three and G groups.  Both are calls of the same functions below.
//
//   dec_conv_kernel:        CausalConv1d.forward (layers/conv_layer.py:146-149), kernel k, dilation d, G groups: output channel
//                           co of group g = co / (C_out / G) sums over that group's input channels ci,
//                             y[b][co][u] = bias[co] + sum_{ci,j} W[co][ci - g C_in/G][j] a(x[b][ci][u - (k-1-j) d]) + res[b][co][u]
//                           One GEMM per group g = blockIdx.z: M = C_out/G, K = (C_in/G) k (kk = ci k + j), N = B T; W transposed
//                           at load to [g][kk][co].  The left zero padding is predicated loads; the residual unit's skip is the
//                           epilogue's `res`.
//   dec_direct_kernel:      the same sum, one thread per output, for conv2 (C_out = 1 or 2), where a 32-row tile is mostly empty.
//   dec_conv_grad_kernel:   dx[b][ci][u] = a'(x[b][ci][u]) sum_{co,j} W[co][ci][j] dy[b][co][u + (k-1-j) d] + dres[b][ci][u]
//                           (indices >= T skipped; co over ci's group).  One GEMM per group: M = C_in/G, K = (C_out/G) k
//                           (kk = co k + j), N = B T; W re-packed to [g][kk][ci].
//                           a'(x) and the skip gradient `dres` are the epilogue.
//   dec_convtr_kernel:      CausalConvTranspose1d.forward (layers/conv_layer.py:189-192) for kernel = 2 stride: replicate padding
//                           by one frame, ConvTranspose1d, crop of one stride at both ends -- in polyphase form
//                             y[b][co][i s + r] = bias[co] + sum_ci W[ci][co][r] a(x[b][ci][i]) + W[ci][co][s + r] a(x[b][ci][max(i-1, 0)])
//                           One GEMM per phase r = blockIdx.z: M = C_out, K = 2 C_in (kk = 2 ci + tap), N = B T; W re-packed to
//                           [r][kk][co].  A phase's stores are strided by s (as DiscGradSrc's are).
//   dec_convtr_grad_kernel: dx[b][ci][i] = a'(x[b][ci][i]) sum_{co, q < 2s} W[ci][co][q] g(co, i, q),
//                             g = [i s + q < T s] dy[b][co][i s + q] + [i == 0 and q >= s] dy[b][co][q - s]
//                           (q < s: this frame's own phase; q >= s: the next frame's second tap; the last term is the replicate
//                           padding's share, which frame 0 collects).  GEMM M = C_in, K = C_out 2s (kk = co 2s + q), N = B T;
//                           W re-packed to [kk][ci].
//   rvq_st_grad_kernel:     the backward of Quantizer.forward in eval mode to z (layers/vq_module.py:83-84, 119-134): the
//                           straight-through step passes dzq through stage 0 only and only vqloss[0] reaches z,
//                             dz = dzq + up_vq[0] 2 (z - q0) / (rows dim),   q0 the stage-0 code of the row.
#include "conv_gemm_f32.h"

namespace adk {

// One layer as both directions see it.  t is the INPUT length; a transposed conv's output has t * stride samples.
struct DecGeom {
    int n_items, c_in, c_out, t, ksz, dil, stride, act;
    int cin_g, cout_g;                              // channels of one group (the transposed conv has one)
    float alpha;
    long long n_cols;                               // n_items * t: GEMM N of every kernel here
};
struct DecConv : DecGeom {                          // x [n_items][c_in][t] -> y [n_items][c_out][t (* stride)]
    const float* x; const float* w; const float* bias; const float* res; float* y;
};
struct DecGrad : DecGeom {                          // dy of y's shape, x -> dx of x's
    const float* dy; const float* x; const float* w; const float* dres; float* dx;
};

// The epilogues: y = v + res, and dx = a'(x) v + dres, res / x / dres at the output element's own offset.
struct DecResStore {
    const float* res; const float* y0;
    __device__ __forceinline__ void operator()(float* dst, float v, int, float) const { *dst = res ? v + res[dst - y0] : v; }
};
struct DecGradStore {
    const float* x; const float* dres; const float* dx0; int act; float alpha;
    __device__ __forceinline__ void operator()(float* dst, float v, int, float) const {
        const long long o = dst - dx0;
        if (act != IN_ACT_NONE) v *= in_dact(x[o], act, alpha);
        *dst = dres ? v + dres[o] : v;
    }
};

// Group g = blockIdx.z of the stride-1 conv: its rows are output channels g C_out/G + m, its K index kk = ci k + j runs over
// the group's own input channels g C_in/G + ci.  Nothing of another group is read or written.
struct DecConvSrc {
    const DecConv& c;
    const int g = blockIdx.z;
    long long xbase = 0;
    int u = -0x40000000;                            // an invalid column fails the bounds test
    __device__ int k_extent() const { return c.cin_g * c.ksz; }
    __device__ int m_extent() const { return c.cout_g; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w + (size_t)g * c.cin_g * c.ksz * c.cout_g; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.t;
            u = (int)(col - item * c.t);
            xbase = (item * c.c_in + (long long)g * c.cin_g) * c.t;
        }
    }
    __device__ float tap(int kk) const {
        const int ci = kk / c.ksz, tt = u - (c.ksz - 1 - (kk - ci * c.ksz)) * c.dil;
        const bool ok = kk < c.cin_g * c.ksz && tt >= 0;
        return ok ? in_act(c.x[xbase + (long long)ci * c.t + tt], c.act, c.alpha) : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.t;
        return c.y + (item * c.c_out + (long long)g * c.cout_g) * c.t + (n - item * c.t);
    }
    __device__ long long out_stride() const { return c.t; }
    __device__ int bias_index(int m) const { return g * c.cout_g + m; }
};

// Group g = blockIdx.z of its backward: rows are input channels g C_in/G + m, kk = co k + j runs over the group's own dy rows.
struct DecConvGradSrc {
    const DecGrad& c;
    const int g = blockIdx.z;
    long long ybase = 0;
    int u = 0x40000000;                             // an invalid column fails the bounds test
    __device__ int k_extent() const { return c.cout_g * c.ksz; }
    __device__ int m_extent() const { return c.cin_g; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w + (size_t)g * c.cout_g * c.ksz * c.cin_g; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.t;
            u = (int)(col - item * c.t);
            ybase = (item * c.c_out + (long long)g * c.cout_g) * c.t;
        }
    }
    __device__ float tap(int kk) const {
        const int co = kk / c.ksz, tt = u + (c.ksz - 1 - (kk - co * c.ksz)) * c.dil;
        const bool ok = kk < c.cout_g * c.ksz && tt < c.t;
        return ok ? c.dy[ybase + (long long)co * c.t + tt] : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.t;
        return c.dx + (item * c.c_in + (long long)g * c.cin_g) * c.t + (n - item * c.t);
    }
    __device__ long long out_stride() const { return c.t; }
    __device__ int bias_index(int m) const { return m; }
};

// Phase r = blockIdx.z of the transposed conv: K index kk = 2 ci + tap, tap 0 reads frame i, tap 1 frame max(i - 1, 0).
struct DecConvTrSrc {
    const DecConv& c;
    const int r = blockIdx.z;
    long long xbase = 0;
    int i = 0;
    bool valid = false;
    __device__ int k_extent() const { return 2 * c.c_in; }
    __device__ int m_extent() const { return c.c_out; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w + (size_t)r * 2 * c.c_in * c.c_out; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.t;
            i = (int)(col - item * c.t);
            xbase = item * c.c_in * c.t;
            valid = true;
        }
    }
    __device__ float tap(int kk) const {
        const int ci = kk >> 1, f = (kk & 1) ? max(i - 1, 0) : i;
        const bool ok = valid && kk < 2 * c.c_in;
        return ok ? in_act(c.x[xbase + (long long)ci * c.t + f], c.act, c.alpha) : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.t, f = n - item * c.t;
        return c.y + (item * c.c_out * c.t + f) * c.stride + r;
    }
    __device__ long long out_stride() const { return (long long)c.t * c.stride; }
    __device__ int bias_index(int m) const { return m; }
};

// K index kk = co 2s + q: output sample i s + q of channel co, and for frame 0 the replicate padding's share q - s.
struct DecConvTrGradSrc {
    const DecGrad& c;
    const int k2 = 2 * c.stride;
    const long long ts = (long long)c.t * c.stride;
    long long ybase = 0, p0 = 0;
    int i = 0;
    bool valid = false;
    __device__ int k_extent() const { return c.c_out * k2; }
    __device__ int m_extent() const { return c.c_in; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.t;
            i = (int)(col - item * c.t);
            p0 = (long long)i * c.stride;
            ybase = item * c.c_out * ts;
            valid = true;
        }
    }
    __device__ float tap(int kk) const {
        const int co = kk / k2, q = kk - co * k2;
        if (!valid || kk >= c.c_out * k2) return 0.f;
        const float* row = c.dy + ybase + (long long)co * ts;
        float v = p0 + q < ts ? row[p0 + q] : 0.f;
        if (i == 0 && q >= c.stride) v += row[q - c.stride];
        return v;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.t;
        return c.dx + item * c.c_in * c.t + (n - item * c.t);
    }
    __device__ long long out_stride() const { return c.t; }
    __device__ int bias_index(int m) const { return m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void dec_conv_kernel(DecConv c) {
    DecConvSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, c.bias, CG_ACT_NONE, 0.f, DecResStore{c.res, c.y});
}
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void dec_conv_grad_kernel(DecGrad c) {
    DecConvGradSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, nullptr, CG_ACT_NONE, 0.f, DecGradStore{c.x, c.dres, c.dx, c.act, c.alpha});
}
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void dec_convtr_kernel(DecConv c) {
    DecConvTrSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, c.bias, CG_ACT_NONE, 0.f, DecResStore{nullptr, c.y});
}
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void dec_convtr_grad_kernel(DecGrad c) {
    DecConvTrGradSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, nullptr, CG_ACT_NONE, 0.f, DecGradStore{c.x, nullptr, c.dx, c.act, c.alpha});
}

// One output per thread, summed in the GEMM's order kk = ci k + j.  w is the reference's layout [c_out][c_in][kernel]; one group.
__global__ __launch_bounds__(CG_THREADS) void dec_direct_kernel(DecConv c) {
    const long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
    if (o >= c.n_cols * c.c_out) return;
    const int u = (int)(o % c.t);
    const long long q = o / c.t;
    const int co = (int)(q % c.c_out);
    const float* __restrict__ xb = c.x + (q / c.c_out) * c.c_in * c.t;
    const float* __restrict__ wr = c.w + (size_t)co * c.c_in * c.ksz;
    float s = 0.f;
    for (int ci = 0; ci < c.c_in; ++ci)
        for (int j = 0; j < c.ksz; ++j) {
            const int tt = u - (c.ksz - 1 - j) * c.dil;
            if (tt >= 0) s = fmaf(wr[ci * c.ksz + j], in_act(xb[(long long)ci * c.t + tt], c.act, c.alpha), s);
        }
    s += c.bias ? c.bias[co] : 0.f;
    c.y[o] = c.res ? s + c.res[o] : s;
}

// One dz element per thread; z, dzq, dz are [n_items][dim][t], row (item, frame) has index idx[item * t + frame].
__global__ __launch_bounds__(CG_THREADS) void rvq_st_grad_kernel(const float* __restrict__ dzq, const float* __restrict__ up_vq,
                                                                 const float* __restrict__ z, const float* __restrict__ codebook,
                                                                 const int64_t* __restrict__ idx, float* __restrict__ dz, int dim,
                                                                 int t, int size, long long total, double scale, int* flags) {
    const float coef = up_vq ? (float)((double)up_vq[0] * scale) : 0.f;
    for (long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x; o < total; o += (long long)gridDim.x * CG_THREADS) {
        const int f = (int)(o % t);
        const long long q = o / t;
        const int ch = (int)(q % dim);
        long long i = idx[(q / dim) * t + f];
        if (i < 0 || i >= size) { atomicOr(flags, 1); i = 0; }       // as adk_rvq_lookup reports a bad index
        const float d = coef * (z[o] - codebook[i * dim + ch]);
        dz[o] = dzq ? dzq[o] + d : d;
    }
}

// The checks the conv entry points make of a layer, f the entry point's name, and its geometry.  max_act is the largest act the
// entry point takes: IN_ACT_ELU for adk_dec_*, IN_ACT_LEAKY for adk_voc_*.
static int dec_geometry(const std::string& f, int n_items, int c_in, int t, int c_out, int kernel, int dil, int stride, int groups,
                        int act, int max_act, float alpha, DecGeom& g) {
    if (n_items < 0 || c_in <= 0 || t <= 0 || c_out <= 0 || kernel <= 0 || dil <= 0 || stride <= 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, t, c_out, kernel, dilation / stride > 0");
    if (groups < 1 || c_in % groups || c_out % groups)
        return fail(ADK_ERR_ARG, f + ": need groups >= 1 that divides c_in and c_out");
    if (act < IN_ACT_NONE || act > max_act)
        return fail(ADK_ERR_ARG, f + (max_act == IN_ACT_ELU ? ": act must be 0 (none) or 1 (ELU)" : ": act must be 0 (none), 1 (ELU) or 2 (LeakyReLU)"));
    if (act != IN_ACT_NONE && !(alpha == alpha)) return fail(ADK_ERR_ARG, f + ": alpha is NaN");
    const long long n_cols = (long long)n_items * t;
    // the whole layer's extents bound a group's; a group is one z of the grid
    if ((long long)(kernel - 1) * dil >= (1LL << 30) || t >= (1 << 30) || (long long)t * stride >= (1LL << 40) ||
        (long long)c_in * kernel >= (1LL << 30) || (long long)c_out * kernel >= (1LL << 30) || (n_cols + 31) / 32 >= (1LL << 31) ||
        (c_in + 31) / 32 > 65535 || (c_out + 31) / 32 > 65535 || stride > 65535 || groups > 65535)
        return fail(ADK_ERR_ARG, f + ": layer too large");
    g.n_items = n_items; g.c_in = c_in; g.c_out = c_out; g.t = t; g.ksz = kernel; g.dil = dil; g.stride = stride; g.act = act;
    g.cin_g = c_in / groups; g.cout_g = c_out / groups; g.alpha = alpha; g.n_cols = n_cols;
    return ADK_OK;
}

// The tile follows M (of one group) as in disc.hip: 128 x 128 from M >= 128, 64 x 128 from M >= 64, else 32 x 128; z = phases or groups.
#define DEC_LAUNCH(kernel, c, m, nz, s)                                                                                  \
    do {                                                                                                                 \
        const unsigned nx128 = (unsigned)(((c).n_cols + 127) / 128);                                                      \
        if ((m) >= 128) hipLaunchKernelGGL((kernel<2, 2, 2, 2>), dim3(nx128, ((m) + 127) / 128, nz), dim3(CG_THREADS), 0, s, c); \
        else if ((m) >= 64) hipLaunchKernelGGL((kernel<2, 2, 1, 2>), dim3(nx128, ((m) + 63) / 64, nz), dim3(CG_THREADS), 0, s, c); \
        else hipLaunchKernelGGL((kernel<1, 4, 1, 1>), dim3(nx128, ((m) + 31) / 32, nz), dim3(CG_THREADS), 0, s, c);      \
    } while (0)

// The four layer calls; adk_dec_* and adk_voc_* differ in max_act and in the groups they pass.
static int dec_conv(const std::string& f, int max_act, const float* x, const float* w, const float* bias, const float* res, float* y,
                    int n_items, int c_in, int t, int c_out, int kernel, int dilation, int groups, int act, float alpha, int impl,
                    void* stream) {
    DecConv c;
    int rc = dec_geometry(f, n_items, c_in, t, c_out, kernel, dilation, 1, groups, act, max_act, alpha, c);
    if (rc != ADK_OK) return rc;
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, f + ": impl must be 1 (direct) or 2 (gemm)");
    if (impl == CG_IMPL_DIRECT && groups != 1) return fail(ADK_ERR_ARG, f + ": impl 1 (direct) is for one group");
    rc = check_pointers(f, "x/w/bias/res/y", n_items > 0 && (!x || !w || !y), {x, w, bias, res, y});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.x = x; c.w = w; c.bias = bias; c.res = res; c.y = y;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    if (impl == CG_IMPL_DIRECT) {
        const long long nb = (c.n_cols * c_out + CG_THREADS - 1) / CG_THREADS;
        if (nb >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": layer too large for the direct kernel");
        hipLaunchKernelGGL(dec_direct_kernel, dim3((unsigned)nb), dim3(CG_THREADS), 0, s, c);
    } else {
        DEC_LAUNCH(dec_conv_kernel, c, c.cout_g, groups, s);
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

static int dec_conv_grad(const std::string& f, int max_act, const float* dy, const float* x, const float* w, const float* dres,
                         float* dx, int n_items, int c_in, int t, int c_out, int kernel, int dilation, int groups, int act,
                         float alpha, void* stream) {
    DecGrad c;
    int rc = dec_geometry(f, n_items, c_in, t, c_out, kernel, dilation, 1, groups, act, max_act, alpha, c);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/x/w/dres/dx", n_items > 0 && (!dy || !w || !dx || (act != IN_ACT_NONE && !x)), {dy, x, w, dres, dx});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.dy = dy; c.x = x; c.w = w; c.dres = dres; c.dx = dx;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    DEC_LAUNCH(dec_conv_grad_kernel, c, c.cin_g, groups, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

static int dec_convtr(const std::string& f, int max_act, const float* x, const float* w, const float* bias, float* y, int n_items,
                      int c_in, int t, int c_out, int kernel, int stride, int act, float alpha, void* stream) {
    DecConv c;
    int rc = dec_geometry(f, n_items, c_in, t, c_out, kernel, 1, stride, 1, act, max_act, alpha, c);
    if (rc != ADK_OK) return rc;
    if ((long long)kernel != 2LL * stride) return fail(ADK_ERR_ARG, f + ": kernel must be 2 * stride");
    rc = check_pointers(f, "x/w/bias/y", n_items > 0 && (!x || !w || !y), {x, w, bias, y});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.x = x; c.w = w; c.bias = bias; c.res = nullptr; c.y = y;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    DEC_LAUNCH(dec_convtr_kernel, c, c_out, stride, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

static int dec_convtr_grad(const std::string& f, int max_act, const float* dy, const float* x, const float* w, float* dx, int n_items,
                           int c_in, int t, int c_out, int kernel, int stride, int act, float alpha, void* stream) {
    DecGrad c;
    int rc = dec_geometry(f, n_items, c_in, t, c_out, kernel, 1, stride, 1, act, max_act, alpha, c);
    if (rc != ADK_OK) return rc;
    if ((long long)kernel != 2LL * stride) return fail(ADK_ERR_ARG, f + ": kernel must be 2 * stride");
    rc = check_pointers(f, "dy/x/w/dx", n_items > 0 && (!dy || !w || !dx || (act != IN_ACT_NONE && !x)), {dy, x, w, dx});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.dy = dy; c.x = x; c.w = w; c.dres = nullptr; c.dx = dx;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    DEC_LAUNCH(dec_convtr_grad_kernel, c, c_in, 1, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_dec_conv(const float* x, const float* w, const float* bias, const float* res, float* y, int32_t n_items,
                            int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t act, float alpha,
                            int32_t impl, void* stream) {
    return dec_conv("adk_dec_conv", IN_ACT_ELU, x, w, bias, res, y, n_items, c_in, t, c_out, kernel, dilation, 1, act, alpha, impl, stream);
}
extern "C" int adk_dec_conv_grad(const float* dy, const float* x, const float* w, const float* dres, float* dx, int32_t n_items,
                                 int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t act,
                                 float alpha, void* stream) {
    return dec_conv_grad("adk_dec_conv_grad", IN_ACT_ELU, dy, x, w, dres, dx, n_items, c_in, t, c_out, kernel, dilation, 1, act, alpha, stream);
}
extern "C" int adk_dec_convtr(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in,
                              int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream) {
    return dec_convtr("adk_dec_convtr", IN_ACT_ELU, x, w, bias, y, n_items, c_in, t, c_out, kernel, stride, act, alpha, stream);
}
extern "C" int adk_dec_convtr_grad(const float* dy, const float* x, const float* w, float* dx, int32_t n_items, int32_t c_in,
                                   int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha,
                                   void* stream) {
    return dec_convtr_grad("adk_dec_convtr_grad", IN_ACT_ELU, dy, x, w, dx, n_items, c_in, t, c_out, kernel, stride, act, alpha, stream);
}

extern "C" int adk_voc_conv(const float* x, const float* w, const float* bias, const float* res, float* y, int32_t n_items,
                            int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups, int32_t act,
                            float alpha, int32_t impl, void* stream) {
    return dec_conv("adk_voc_conv", IN_ACT_LEAKY, x, w, bias, res, y, n_items, c_in, t, c_out, kernel, dilation, groups, act, alpha, impl, stream);
}
extern "C" int adk_voc_conv_grad(const float* dy, const float* x, const float* w, const float* dres, float* dx, int32_t n_items,
                                 int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups,
                                 int32_t act, float alpha, void* stream) {
    return dec_conv_grad("adk_voc_conv_grad", IN_ACT_LEAKY, dy, x, w, dres, dx, n_items, c_in, t, c_out, kernel, dilation, groups, act, alpha, stream);
}
extern "C" int adk_voc_convtr(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in,
                              int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream) {
    return dec_convtr("adk_voc_convtr", IN_ACT_LEAKY, x, w, bias, y, n_items, c_in, t, c_out, kernel, stride, act, alpha, stream);
}
extern "C" int adk_voc_convtr_grad(const float* dy, const float* x, const float* w, float* dx, int32_t n_items, int32_t c_in,
                                   int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha,
                                   void* stream) {
    return dec_convtr_grad("adk_voc_convtr_grad", IN_ACT_LEAKY, dy, x, w, dx, n_items, c_in, t, c_out, kernel, stride, act, alpha, stream);
}

extern "C" int adk_rvq_st_grad(const float* dzq, const float* up_vq, const float* z, const float* codebook, const int64_t* idx,
                               float* dz, int32_t n_items, int32_t dim, int32_t t, int32_t size, void* stream) {
    const std::string f = "adk_rvq_st_grad";
    if (n_items < 0 || dim <= 0 || t <= 0 || size <= 0) return fail(ADK_ERR_ARG, f + ": need n_items >= 0, dim, t, size > 0");
    const long long rows = (long long)n_items * t;
    if (rows >= (1LL << 31) || (long long)size * dim >= (1LL << 31) || rows * dim >= (1LL << 40))
        return fail(ADK_ERR_ARG, f + ": extents too large");
    if (n_items > 0 && (!z || !codebook || !idx || !dz)) return fail(ADK_ERR_ARG, f + ": null pointer");
    int rc = check_pointers(f, "dzq/up_vq/z/codebook/dz", false, {dzq, up_vq, z, codebook, dz});
    if (rc != ADK_OK) return rc;
    if (reinterpret_cast<uintptr_t>(idx) & 7) return fail(ADK_ERR_ARG, f + ": idx must be 8-byte aligned");
    if (n_items == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dz));
    const long long total = rows * dim;
    const int nb = (int)std::min<long long>((total + CG_THREADS - 1) / CG_THREADS, 8192);
    hipLaunchKernelGGL(rvq_st_grad_kernel, dim3(nb), dim3(CG_THREADS), 0, s, dzq, up_vq, z, codebook, idx, dz, (int)dim, (int)t,
                       (int)size, total, 2.0 / (double)total, flags_word());
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
