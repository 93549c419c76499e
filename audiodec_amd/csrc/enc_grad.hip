// The encoder's training half: the strided down-sampling conv (models/autoencoder/modules/encoder.py:62-68) forward and backward
// to its input, and the gradient of a causal conv with respect to its weight and bias, for every layer kind of the encoder.
// Exact f32 on v_mfma_f32_32x32x2_f32; every output element is written once by one thread or one accumulator, nothing is added
// atomically, and every split of a sum is a function of the shape alone: forward and gradients are bitwise reproducible.
//
// a is a conv's INPUT activation as in dec_grad.hip (conv_gemm_f32.h's in_act): none, ELU(alpha) or LeakyReLU(alpha).  adk_conv_wgrad
// (encoder and symmetric decoder) takes none or ELU and one group, adk_voc_conv_wgrad (the HiFi-GAN vocoder) all three and G groups.
// k kernel, d dilation, s stride, T the input length, T_out = (T - 1) / s + 1; an index outside [0, T) or [0, T_out) is skipped
// (the causal left padding is predicated loads).
//
//   enc_down_kernel:       CausalConv1d.forward for k = 2s, d = 1, no input activation:
//                            y[b][co][u] = bias[co] + sum_{ci,j} W[co][ci][j] x[b][ci][u s - (k-1-j)]
//                          conv_gemm_f32's core: M = C_out, K = C_in k (kk = ci k + j), N = B T_out; W is [kk][co].
//   enc_down_grad_kernel:  dx[b][ci][v] = sum_co sum_{j : (v+k-1-j) % s == 0, u = (v+k-1-j)/s < T_out} W[co][ci][j] dy[b][co][u]
//                          For k = 2s, v = q s + r has the two taps j0 = (r + s - 1) % s and j0 + s, which read
//                          u0 = q + (r ? 2 : 1) and u0 - 1.  One GEMM per phase r = blockIdx.z: M = C_in, K = 2 C_out
//                          (kk = 2 co + tap), N = B count_r, count_r the v < T of phase r; W re-packed to [r][kk][ci].  A phase's
//                          stores are strided by s.  No structural zero is multiplied.
//   wgrad_kernel:          dW[co][ci][j] = sum_{b,u} dy[b][co][u] a(x[b][g C_in/G + ci][u s - (k-1-j) d]),  db[co] = sum_{b,u} dy[b][co][u]
//                          for co of group g = co / (C_out/G) and ci < C_in/G.  wgrad_gemm.h's core, one GEMM per group: M = C_out/G,
//                          N = (C_in/G) k + 1 (n = ci k + j; the last column's tap is 1: db, left out when db is not asked for, which
//                          saves the 1x1 convs of 2^n channels a whole column tile), reduction over rho = b T_out + u, along which
//                          dy and x are contiguous.  blockIdx.z = g S + slice (wgrad_plan); the workspace is [slice][g C_out/G + m][n]:
//                          rows of all groups side by side, the layout of dW itself (the reference's: m (C_in k) + n), which
//                          wgrad_gemm.h's fold then writes.
#include "wgrad_gemm.h"

namespace adk {

struct EncDown {                                    // x [n_items][c_in][t] -> y [n_items][c_out][t_out]
    int n_items, c_in, c_out, t, t_out, ksz, stride;
    long long n_cols;                               // n_items * t_out
    const float* x; const float* w; const float* bias; float* y;
};
struct EncDownGrad {                                // dy [n_items][c_out][t_out] -> dx [n_items][c_in][t]
    int n_items, c_in, c_out, t, t_out, ksz, stride;
    long long n_cols;
    const float* dy; const float* w; float* dx;
};

struct EncPlainStore {
    __device__ __forceinline__ void operator()(float* dst, float v, int, float) const { *dst = v; }
};

struct EncDownSrc {
    const EncDown& c;
    long long xbase = 0;
    int p = -0x40000000;                            // u s; an invalid column fails the bounds test
    __device__ int k_extent() const { return c.c_in * c.ksz; }
    __device__ int m_extent() const { return c.c_out; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.t_out;
            p = (int)(col - item * c.t_out) * c.stride;
            xbase = item * c.c_in * c.t;
        }
    }
    __device__ float tap(int kk) const {
        const int ci = kk / c.ksz, tt = p - (c.ksz - 1 - (kk - ci * c.ksz));
        const bool ok = kk < c.c_in * c.ksz && tt >= 0;                 // tt <= u s <= t - 1
        return ok ? c.x[xbase + (long long)ci * c.t + tt] : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.t_out;
        return c.y + item * c.c_out * c.t_out + (n - item * c.t_out);
    }
    __device__ long long out_stride() const { return c.t_out; }
    __device__ int bias_index(int m) const { return m; }
};

// Phase r = blockIdx.z of the backward: columns are the v = q s + r < t of every item; kk = 2 co + tap reads u0 - tap.
struct EncDownGradSrc {
    const EncDownGrad& c;
    const int r = blockIdx.z;
    const int cnt = phase_count(c.t, c.stride, r);
    const int lead = r ? 2 : 1;
    long long ybase = 0;
    int q = 0;
    bool valid = false;
    __device__ int k_extent() const { return 2 * c.c_out; }
    __device__ int m_extent() const { return c.c_in; }
    __device__ long long n_cols() const { return (long long)c.n_items * cnt; }
    __device__ const float* weights() const { return c.w + (size_t)r * 2 * c.c_out * c.c_in; }
    __device__ void column(long long col) {
        if (col < n_cols()) {
            const long long item = col / cnt;
            q = (int)(col - item * cnt);
            ybase = item * c.c_out * c.t_out;
            valid = true;
        }
    }
    __device__ float tap(int kk) const {
        const int co = kk >> 1, u = q + lead - (kk & 1);
        const bool ok = valid && kk < 2 * c.c_out && u < c.t_out;
        return ok ? c.dy[ybase + (long long)co * c.t_out + u] : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / cnt;
        return c.dx + item * c.c_in * c.t + (n - item * cnt) * c.stride + r;
    }
    __device__ long long out_stride() const { return c.t; }
    __device__ int bias_index(int m) const { return m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void enc_down_kernel(EncDown c) {
    EncDownSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, c.bias, CG_ACT_NONE, 0.f, EncPlainStore{});
}
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void enc_down_grad_kernel(EncDownGrad c) {
    EncDownGradSrc src{c};
    conv_gemm_f32<WM, WN, TM, TN>(src, nullptr, CG_ACT_NONE, 0.f, EncPlainStore{});
}

// ---- the weight gradient ----
struct WGrad {
    int n_items, c_in, c_out, t, t_out, ksz, dil, stride, act;
    float alpha;
    int cin_g, cout_g;                              // channels of one group
    int ck;                                         // cin_g * ksz: columns 0 .. ck - 1 are dW's, column ck is db's
    int nc_live;                                    // columns computed: ck + 1, or ck when db is not asked for
    int red;                                        // n_items * t_out: the reduction length
    int steps_per, slices;                          // 32-deep steps of one slice, and S
    const float* dy; const float* x; float* ws;     // ws [slices][c_out][ck + 1]
};                                                  // the grid's z is groups * slices

// wgrad_gemm.h's Stage of the causal conv: A is dy (rows of the group), B the activated x at tap (ci, j), or 1 in db's column.
template <int BM, int BN>
struct WGradStage {
    static constexpr int A_PER = BM / WG_ROWS, B_PER = BN / WG_ROWS;
    const int kr = threadIdx.x % WG_KT, row0 = threadIdx.x / WG_KT;    // this thread's reduction offset in a step, and its first row
    const int m0, row_g;                                        // the tile's first row in the group, the group's first dy row
    int xoff[B_PER], need[B_PER];                               // per column: x offset of tap (ci, j) inside an item, the u s it needs at least
    unsigned bias_col = 0;                                      // bit i: this thread's column i is db's
    float ra[A_PER], rb[B_PER];
    unsigned amask = 0, bmask = 0;
    bool live = false;

    __device__ __forceinline__ WGradStage(const WGrad& c, int grp, int m0_, int n0) : m0(m0_), row_g(grp * c.cout_g) {
        const int ch_g = grp * c.cin_g;                         // the group's first x channel
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int n = n0 + row0 + i * WG_ROWS;
            const bool tap = n < c.ck;                          // the bias column and columns past it read no x
            const int ci = n / c.ksz, back = (c.ksz - 1 - (n - ci * c.ksz)) * c.dil;
            xoff[i] = tap ? (ch_g + ci) * c.t - back : 0;
            need[i] = tap ? back : 0x7fffffff;
            bias_col |= (n == c.ck && n < c.nc_live) ? 1u << i : 0u;
        }
    }
    __device__ __forceinline__ void prepare(float*, int) {}
    // clamped address: element 0 of the item (a step exists only when the operands do)
    __device__ __forceinline__ void load(const WGrad& c, int step) {
        const int rho = step * WG_KT + kr;
        live = rho < c.red;
        const int item = live ? rho / c.t_out : 0, u = live ? rho - item * c.t_out : 0;
        const float* __restrict__ dyb = c.dy + (long long)item * c.c_out * c.t_out + u;
        const float* __restrict__ xb = c.x + (long long)item * c.c_in * c.t;
        const int p = u * c.stride;
        amask = bmask = 0;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int m = m0 + row0 + i * WG_ROWS;
            const bool ok = live && m < c.cout_g;
            ra[i] = dyb[ok ? (long long)(row_g + m) * c.t_out : 0];
            amask |= ok ? 1u << i : 0u;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const bool ok = live && p >= need[i];
            rb[i] = xb[ok ? xoff[i] + p : 0];
            bmask |= ok ? 1u << i : 0u;
        }
    }
    __device__ __forceinline__ void store(const WGrad& c, float* As, int LDA, float* Bs, int LDB) const {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) As[kr * LDA + row0 + i * WG_ROWS] = (amask >> i & 1) ? ra[i] : 0.f;
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const float one = (live && (bias_col >> i & 1)) ? 1.f : 0.f;
            Bs[kr * LDB + row0 + i * WG_ROWS] = (bmask >> i & 1) ? in_act(rb[i], c.act, c.alpha) : one;
        }
    }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void wgrad_kernel(WGrad c) {
    const int grp = blockIdx.z / c.slices, slice = blockIdx.z - grp * c.slices;
    WGradStage<WM * TM * 32, WN * TN * 32> stage(c, grp, blockIdx.y * (WM * TM * 32), blockIdx.x * (WN * TN * 32));
    wgrad_gemm<WM, WN, TM, TN>(stage, c, c.red, c.steps_per, slice, c.cout_g, c.nc_live,
                               c.ws + ((size_t)slice * c.c_out + grp * c.cout_g) * (c.ck + 1), c.ck + 1);
}

// ---- host ----
static int enc_down_geometry(const std::string& f, int n_items, int c_in, int t, int c_out, int kernel, int stride, int& t_out) {
    if (n_items < 0 || c_in <= 0 || t <= 0 || c_out <= 0 || kernel <= 0 || stride <= 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, t, c_out, kernel, stride > 0");
    if ((long long)kernel != 2LL * stride) return fail(ADK_ERR_ARG, f + ": kernel must be 2 * stride");
    t_out = (t - 1) / stride + 1;
    const long long n_cols = (long long)n_items * t_out;
    if (t >= (1 << 30) || stride > 65535 || (long long)c_in * kernel >= (1LL << 30) || (long long)c_out * kernel >= (1LL << 30) ||
        (n_cols + 31) / 32 >= (1LL << 31) || (c_in + 31) / 32 > 65535 || (c_out + 31) / 32 > 65535)
        return fail(ADK_ERR_ARG, f + ": layer too large");
    return ADK_OK;
}

// The tile follows M as DEC_LAUNCH's: 128 x 128 from M >= 128, 64 x 128 from M >= 64, else 32 x 128; z = phases.
#define ENC_LAUNCH(kernel, c, m, phases, s)                                                                              \
    do {                                                                                                                 \
        const unsigned nx128 = (unsigned)(((c).n_cols + 127) / 128);                                                      \
        if ((m) >= 128) hipLaunchKernelGGL((kernel<2, 2, 2, 2>), dim3(nx128, ((m) + 127) / 128, phases), dim3(CG_THREADS), 0, s, c); \
        else if ((m) >= 64) hipLaunchKernelGGL((kernel<2, 2, 1, 2>), dim3(nx128, ((m) + 63) / 64, phases), dim3(CG_THREADS), 0, s, c); \
        else hipLaunchKernelGGL((kernel<1, 4, 1, 1>), dim3(nx128, ((m) + 31) / 32, phases), dim3(CG_THREADS), 0, s, c);  \
    } while (0)

// The weight gradient's checks and geometry; the slice rule is wgrad_gemm.h's wgrad_slices with the tiles of all groups.  max_act
// is the largest act the entry point takes: IN_ACT_ELU for adk_conv_wgrad, IN_ACT_LEAKY for adk_voc_conv_wgrad.
static int wgrad_plan(const std::string& f, int n_items, int c_in, int t, int c_out, int kernel, int dil, int stride, int groups,
                      int act, int max_act, float alpha, WGrad& g, long long& ws_bytes) {
    if (n_items < 0 || c_in <= 0 || t <= 0 || c_out <= 0 || kernel <= 0 || dil <= 0 || stride <= 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, t, c_out, kernel, dilation, stride > 0");
    if (groups < 1 || c_in % groups || c_out % groups)
        return fail(ADK_ERR_ARG, f + ": need groups >= 1 that divides c_in and c_out");
    if (const int rc = wgrad_check_in_act(f, act, max_act, alpha)) return rc;
    const int t_out = (t - 1) / stride + 1, cin_g = c_in / groups, cout_g = c_out / groups;
    const long long red = (long long)n_items * t_out, ck = (long long)cin_g * kernel;
    // the whole layer's c_in * kernel bounds a group's ck; c_in * t is the x offset of the last group's last channel
    if (t >= (1 << 30) || (long long)(kernel - 1) * dil >= (1LL << 30) || (long long)c_in * kernel >= (1LL << 30) ||
        (long long)c_in * t >= (1LL << 31) || red >= (1LL << 31) - WG_KT || (long long)c_out * (ck + 1) >= (1LL << 31) ||
        (c_out + 31) / 32 > 65535)
        return fail(ADK_ERR_ARG, f + ": layer too large");
    long long steps_per = 1, slices = 1;
    wgrad_slices(wgrad_tiles(groups, cout_g, ck + 1), (red + WG_KT - 1) / WG_KT, steps_per, slices);
    if (groups * slices > 65535) return fail(ADK_ERR_ARG, f + ": layer too large (groups * slices is the grid's z)");
    g.n_items = n_items; g.c_in = c_in; g.c_out = c_out; g.t = t; g.t_out = t_out; g.ksz = kernel; g.dil = dil; g.stride = stride;
    g.act = act; g.alpha = alpha; g.cin_g = cin_g; g.cout_g = cout_g; g.ck = (int)ck; g.nc_live = (int)ck + 1; g.red = (int)red;
    g.steps_per = (int)steps_per; g.slices = (int)slices;
    ws_bytes = slices * c_out * (ck + 1) * 4;
    return ADK_OK;
}

static int conv_wgrad_plan(const std::string& f, int n_items, int c_in, int t, int c_out, int kernel, int dilation, int stride,
                           int groups, int64_t* workspace_bytes, int32_t* slices) {
    WGrad g;
    long long bytes = 0;
    const int rc = wgrad_plan(f, n_items, c_in, t, c_out, kernel, dilation, stride, groups, IN_ACT_NONE, IN_ACT_NONE, 0.f, g, bytes);
    if (rc != ADK_OK) return rc;
    if (workspace_bytes) *workspace_bytes = bytes;
    if (slices) *slices = g.slices;
    return ADK_OK;
}

static int conv_wgrad(const std::string& f, int max_act, const float* dy, const float* x, float* dw, float* db, void* workspace,
                      int n_items, int c_in, int t, int c_out, int kernel, int dilation, int stride, int groups, int act, float alpha,
                      void* stream) {
    WGrad c;
    long long bytes = 0;
    int rc = wgrad_plan(f, n_items, c_in, t, c_out, kernel, dilation, stride, groups, act, max_act, alpha, c, bytes);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/x/dw/db/workspace", !dw || !workspace || (n_items > 0 && (!dy || !x)), {dy, x, dw, db, workspace});
    if (rc != ADK_OK) return rc;
    c.dy = dy; c.x = x; c.ws = static_cast<float*>(workspace);
    c.nc_live = db ? c.ck + 1 : c.ck;                          // without db its column is not computed
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dw));
    WGRAD_LAUNCH(wgrad_kernel, c, c.cout_g, (unsigned)((c.nc_live + 127) / 128), (unsigned)(groups * c.slices), s);
    ADK_HIP_CHECK(hipGetLastError());
    launch_wgrad_fold(c.ws, dw, db, (int)c_out, c.ck, c.slices, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_enc_down(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t t,
                            int32_t c_out, int32_t kernel, int32_t stride, void* stream) {
    const std::string f = "adk_enc_down";
    EncDown c;
    int rc = enc_down_geometry(f, n_items, c_in, t, c_out, kernel, stride, c.t_out);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "x/w/bias/y", n_items > 0 && (!x || !w || !y), {x, w, bias, y});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.n_items = n_items; c.c_in = c_in; c.c_out = c_out; c.t = t; c.ksz = kernel; c.stride = stride;
    c.n_cols = (long long)n_items * c.t_out;
    c.x = x; c.w = w; c.bias = bias; c.y = y;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    ENC_LAUNCH(enc_down_kernel, c, c_out, 1, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_enc_down_grad(const float* dy, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t t, int32_t c_out,
                                 int32_t kernel, int32_t stride, void* stream) {
    const std::string f = "adk_enc_down_grad";
    EncDownGrad c;
    int rc = enc_down_geometry(f, n_items, c_in, t, c_out, kernel, stride, c.t_out);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/w/dx", n_items > 0 && (!dy || !w || !dx), {dy, w, dx});
    if (rc != ADK_OK) return rc;
    if (n_items == 0) return ADK_OK;
    c.n_items = n_items; c.c_in = c_in; c.c_out = c_out; c.t = t; c.ksz = kernel; c.stride = stride;
    c.n_cols = (long long)n_items * c.t_out;                   // phase 0 has the most columns, t_out per item: the grid's x
    c.dy = dy; c.w = w; c.dx = dx;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    ENC_LAUNCH(enc_down_grad_kernel, c, c_in, stride, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation,
                                   int32_t stride, int64_t* workspace_bytes, int32_t* slices) {
    return conv_wgrad_plan("adk_conv_wgrad_plan", n_items, c_in, t, c_out, kernel, dilation, stride, 1, workspace_bytes, slices);
}
extern "C" int adk_conv_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in,
                              int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t stride, int32_t act, float alpha,
                              void* stream) {
    return conv_wgrad("adk_conv_wgrad", IN_ACT_ELU, dy, x, dw, db, workspace, n_items, c_in, t, c_out, kernel, dilation, stride, 1, act,
                      alpha, stream);
}

extern "C" int adk_voc_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation,
                                       int32_t groups, int64_t* workspace_bytes, int32_t* slices) {
    return conv_wgrad_plan("adk_voc_conv_wgrad_plan", n_items, c_in, t, c_out, kernel, dilation, 1, groups, workspace_bytes, slices);
}
extern "C" int adk_voc_conv_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items,
                                  int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups,
                                  int32_t act, float alpha, void* stream) {
    return conv_wgrad("adk_voc_conv_wgrad", IN_ACT_LEAKY, dy, x, dw, db, workspace, n_items, c_in, t, c_out, kernel, dilation, 1, groups,
                      act, alpha, stream);
}
