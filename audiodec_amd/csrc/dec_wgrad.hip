// The decoder's training half: the gradient of CausalConvTranspose1d (layers/conv_layer.py:189-192, kernel = 2 stride) with respect
// to its weight and bias.  The stride-1 convs of the decoder go through enc_grad.hip's adk_conv_wgrad.  Exact f32 on
// v_mfma_f32_32x32x2_f32; every partial is written once by one accumulator, nothing is added atomically, and every split of a sum
// is a function of the shape alone: the gradients are bitwise reproducible.
//
// a is the conv's INPUT activation as in dec_grad.hip (conv_gemm_f32.h's in_act): none, ELU(alpha) or, for adk_voc_convtr_wgrad
// (the HiFi-GAN vocoder's upsampling layers), LeakyReLU(alpha).  s stride, T the input length, T s the output's.  The
// forward (dec_grad.hip's dec_convtr_kernel) is
//   y[b][co][i s + r] = bias[co] + sum_ci W[ci][co][r] a(x[b][ci][i]) + W[ci][co][s + r] a(x[b][ci][max(i-1, 0)])
// so, with q in [0, 2s):
//   dW[ci][co][q] = sum_{b,i} a(x[b][ci][i]) g(b, co, i, q)
//   g             = [i s + q < T s] dy[b][co][i s + q] + [i == 0 and q >= s] dy[b][co][q - s]       (dec_convtr_grad_kernel's operand)
//   db[co]        = sum_{b,u} dy[b][co][u]
//
//   convtr_wgrad_kernel:  wgrad_gemm.h's core with M = C_in, N = C_out 2s (n = co 2s + q), reduction over rho = b T + i, output
//                         m (C_out 2s) + n: the reference's [ci][co][2s], no transpose.  A is x, contiguous along i.  For one co,
//                         the 2s columns of a 32-deep step read the run dy[b][co][i0 s .. (i0 + 33) s), each element twice: element (frame f, phase j < s) is column j of row f
//                         (the first tap) and column s + j of row f - 1 (the second).  The B staging threads run along that run
//                         -- (co, f, j) with j fastest, so a wave's loads are contiguous in time -- and scatter each element to
//                         its two places in Bs[rho][n].  A second-tap slot is written by the element of the NEXT row whatever
//                         item that row is in: it takes that element's value when both are in one item (else the conv's crop
//                         leaves nothing), plus the replicate padding's share dy[b][co][j] when its own row is frame 0.  So every
//                         slot of the tile is written exactly once per step, steps may span items, and T = 1 needs no other path.
//                         Slice blockIdx.z of S (wgrad_gemm.h's rule with this GEMM's tiles) goes to the workspace [slice][m][N + 1];
//                         wgrad_gemm.h's fold adds them.
//   convtr_bias_*_kernel: db is a reduction of its own on reduce_f64.h (an all-ones row of the GEMM would cost the decoder's
//                         channel counts, all multiples of the tile, a whole row of tiles): workgroup (chunk, co) sums its share of
//                         dy[.][co][.] in f64 -- lanes, butterfly, waves in order -- into a slab, one thread per co adds the chunks
//                         in ascending order and rounds once.  The chunk count is a function of the shape only.
#include "reduce_f64.h"
#include "wgrad_gemm.h"

namespace adk {

constexpr int DW_BN = 128;                          // columns of a tile, whatever its rows
constexpr int DW_RUN = WG_KT + 1;                   // frames of dy a step reads per channel: its 32 rows' and the one after
constexpr int DW_B_PER = 12;                        // dy elements a thread stages per step, at most (a stride up to 18 fits)
constexpr int DW_BIAS_CHUNK = 4096, DW_BIAS_MAX_CHUNKS = 64;

struct ConvTrWGrad {
    int n_items, c_in, c_out, t, stride, act;
    float alpha;
    int ts;                                         // t * stride: samples of one output row
    int nn;                                         // c_out * 2 stride: GEMM N; a workspace row has nn + 1 floats (the fold's layout)
    int red;                                        // n_items * t: the reduction length
    int steps_per, slices;                          // 32-deep steps of one slice, and S
    int chunks, chunk_len;                          // db: chunks per channel, and the (b, u) pairs of one
    const float* dy; const float* x; float* ws;     // ws [slices][c_in][nn + 1], then (8-byte aligned) double [c_out][chunks]
};

// wgrad_gemm.h's Stage of the transposed conv: A is the activated x, B the scatter of dy described above.
template <int BM, int BN>
struct ConvTrWGradStage {
    static_assert(BN == DW_BN, "the host's element bound is for 128 columns");
    static constexpr int A_PER = BM / WG_ROWS;
    const int tid = threadIdx.x;
    const int kr = tid % WG_KT, row0 = tid / WG_KT;             // A: this thread's reduction offset in a step, and its first row
    const int m0, s;
    // B: the dy elements this thread stages, e = (co, frame f of the run, phase j), j fastest.  Fixed over the steps: f, the
    // first tap's column in the tile (the second's is s further on) and the element's offset in an item at frame 0.
    int fr_[DW_B_PER], col[DW_B_PER], yoff[DW_B_PER];
    unsigned tap1 = 0, tap2 = 0;                                // bit i: element i's first / second tap is a slot of this tile
    float ra[A_PER], rb[DW_B_PER], re[DW_B_PER];
    unsigned amask = 0, own = 0, same = 0, tgt = 0, ext = 0;

    __device__ __forceinline__ ConvTrWGradStage(const ConvTrWGrad& c, int, int m0_, int n0) : m0(m0_), s(c.stride) {
        const int k2 = 2 * s, co0 = n0 / k2, per_co = DW_RUN * s;
        const int n_el = (min((n0 + BN - 1) / k2, c.c_out - 1) - co0 + 1) * per_co;     // <= DW_B_PER * CG_THREADS (the host checks)
#pragma unroll
        for (int i = 0; i < DW_B_PER; ++i) {
            const int e = tid + i * CG_THREADS;
            const int cl = e / per_co, rem = e - cl * per_co, f = rem / s, j = rem - f * s;
            const int n = (co0 + cl) * k2 + j - n0;
            const bool in = e < n_el;
            fr_[i] = in ? f : 0;
            col[i] = in ? n : 0;
            yoff[i] = in ? (co0 + cl) * c.ts + j : 0;
            tap1 |= (in && f < WG_KT && n >= 0 && n < BN) ? 1u << i : 0u;
            tap2 |= (in && f >= 1 && n + s >= 0 && n + s < BN) ? 1u << i : 0u;
        }
    }
    // the tile's columns past N are no element's slot: zero once
    __device__ __forceinline__ void prepare(float* Bs, int n) {
        for (int o = tid; o < n; o += CG_THREADS) Bs[o] = 0.f;
        __syncthreads();
    }
    // clamped address: element 0 (a step exists only when the operands do)
    __device__ __forceinline__ void load(const ConvTrWGrad& c, int step) {
        const int rho0 = step * WG_KT;
        {
            const int rho = rho0 + kr;
            const bool live = rho < c.red;
            const int item = live ? rho / c.t : 0, i = live ? rho - item * c.t : 0;
            const float* __restrict__ xb = c.x + (long long)item * c.c_in * c.t + i;
            amask = 0;
#pragma unroll
            for (int a = 0; a < A_PER; ++a) {
                const int m = m0 + row0 + a * WG_ROWS;
                const bool ok = live && m < c.c_in;
                ra[a] = xb[ok ? m * c.t : 0];
                amask |= ok ? 1u << a : 0u;
            }
        }
        own = same = tgt = ext = 0;
        const long long item_len = (long long)c.c_out * c.ts;
#pragma unroll
        for (int i = 0; i < DW_B_PER; ++i) {
            // this element's own row rho (its first tap), and the row before it, whose second tap it writes
            const int rho = rho0 + fr_[i];
            const bool live = ((tap1 | tap2) >> i & 1) && rho < c.red;
            const int item = live ? rho / c.t : 0, f = live ? rho - item * c.t : 0;
            const bool inside = live && f >= 1;                                     // the row before is in the same item
            const bool t_live = (tap2 >> i & 1) && rho - 1 < c.red;
            const int t_item = inside ? item : live ? item - 1 : c.n_items - 1;     // the row before: (t_item, t_f)
            const int t_f = inside ? f - 1 : c.t - 1;
            const bool pad = t_live && t_f == 0;                                    // it is a frame 0: the padding's share
            rb[i] = c.dy[live ? item * item_len + yoff[i] + f * s : 0];
            re[i] = c.dy[pad ? t_item * item_len + yoff[i] : 0];
            own |= live ? 1u << i : 0u;
            same |= inside ? 1u << i : 0u;
            tgt |= t_live ? 1u << i : 0u;
            ext |= pad ? 1u << i : 0u;
        }
    }
    __device__ __forceinline__ void store(const ConvTrWGrad& c, float* As, int LDA, float* Bs, int LDB) const {
#pragma unroll
        for (int a = 0; a < A_PER; ++a) As[kr * LDA + row0 + a * WG_ROWS] = (amask >> a & 1) ? in_act(ra[a], c.act, c.alpha) : 0.f;
#pragma unroll
        for (int i = 0; i < DW_B_PER; ++i) {
            if (tap1 >> i & 1) Bs[fr_[i] * LDB + col[i]] = (own >> i & 1) ? rb[i] : 0.f;
            if (tap2 >> i & 1) {
                const float v = ((same >> i & 1) ? rb[i] : 0.f) + ((ext >> i & 1) ? re[i] : 0.f);
                Bs[(fr_[i] - 1) * LDB + col[i] + s] = (tgt >> i & 1) ? v : 0.f;
            }
        }
    }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void convtr_wgrad_kernel(ConvTrWGrad c) {
    const int slice = blockIdx.z;
    ConvTrWGradStage<WM * TM * 32, WN * TN * 32> stage(c, 0, blockIdx.y * (WM * TM * 32), blockIdx.x * (WN * TN * 32));
    wgrad_gemm<WM, WN, TM, TN>(stage, c, c.red, c.steps_per, slice, c.c_in, c.nn, c.ws + (size_t)slice * c.c_in * (c.nn + 1), c.nn + 1);
}

// Workgroup (chunk, co): the (b, u) pairs [chunk * chunk_len, + chunk_len) of channel co, u fastest.
__global__ __launch_bounds__(RED_THREADS) void convtr_bias_partial_kernel(const float* __restrict__ dy, double* __restrict__ slab,
                                                                          int c_out, int ts, int total, int chunk_len) {
    const int co = blockIdx.y, lo = blockIdx.x * chunk_len, hi = min(total, lo + chunk_len);
    double acc[1] = {0.0};
    for (int p = lo + (int)threadIdx.x; p < hi; p += RED_THREADS) {
        const int b = p / ts, u = p - b * ts;
        acc[0] += (double)dy[((long long)b * c_out + co) * ts + u];
    }
    workgroup_partials<1>(acc, slab + (size_t)co * gridDim.x);
}

__global__ __launch_bounds__(RED_THREADS) void convtr_bias_fold_kernel(const double* __restrict__ slab, float* __restrict__ db,
                                                                       int c_out, int chunks) {
    const int co = blockIdx.x * RED_THREADS + threadIdx.x;
    if (co >= c_out) return;
    double s = 0.0;
    for (int z = 0; z < chunks; ++z) s += slab[(size_t)co * chunks + z];
    db[co] = (float)s;
}

// The checks, geometry, slice rule and workspace of the transposed conv's weight gradient.
static int convtr_wgrad_plan(const std::string& f, int n_items, int c_in, int t, int c_out, int kernel, int stride, int act, int max_act,
                             float alpha, ConvTrWGrad& g, long long& ws_floats, long long& ws_bytes) {
    if (n_items < 0 || c_in <= 0 || t <= 0 || c_out <= 0 || kernel <= 0 || stride <= 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, t, c_out, kernel, stride > 0");
    if (const int rc = wgrad_check_in_act(f, act, max_act, alpha)) return rc;
    const long long ts = (long long)t * stride, nn = 2LL * c_out * stride, red = (long long)n_items * t;
    // a tile's columns touch at most (BN - 1) / 2s + 2 channels, each with 33 s elements a step: they must fit the staging registers
    const long long el = stride <= DW_BN ? ((DW_BN - 1) / (2LL * stride) + 2) * DW_RUN * stride : (1LL << 40);
    if (t >= (1 << 30) || el > (long long)DW_B_PER * CG_THREADS || nn >= (1LL << 30) || (long long)c_in * t >= (1LL << 31) ||
        c_out * ts >= (1LL << 31) || n_items * ts >= (1LL << 31) || red >= (1LL << 31) - 2 * WG_KT ||
        c_in * (nn + 1) >= (1LL << 31) || (c_in + 31) / 32 > 65535 || c_out > 65535)
        return fail(ADK_ERR_ARG, f + ": layer too large");
    if ((long long)kernel != 2LL * stride) return fail(ADK_ERR_ARG, f + ": kernel must be 2 * stride");
    long long steps_per = 1, slices = 1;
    wgrad_slices(wgrad_tiles(1, c_in, nn), (red + WG_KT - 1) / WG_KT, steps_per, slices);
    const long long total = n_items * ts;
    const long long want = std::max<long long>(1, std::min<long long>(DW_BIAS_MAX_CHUNKS, (total + DW_BIAS_CHUNK - 1) / DW_BIAS_CHUNK));
    const long long chunk_len = std::max<long long>(1, (total + want - 1) / want);
    const long long chunks = std::max<long long>(1, (total + chunk_len - 1) / chunk_len);
    g.n_items = n_items; g.c_in = c_in; g.c_out = c_out; g.t = t; g.stride = stride; g.act = act; g.alpha = alpha;
    g.ts = (int)ts; g.nn = (int)nn; g.red = (int)red; g.steps_per = (int)steps_per; g.slices = (int)slices;
    g.chunks = (int)chunks; g.chunk_len = (int)chunk_len;
    ws_floats = (slices * c_in * (nn + 1) + 1) / 2 * 2;         // the f64 slab after it stays 8-byte aligned
    ws_bytes = ws_floats * 4 + chunks * c_out * 8;
    return ADK_OK;
}

// adk_convtr_wgrad (max_act IN_ACT_ELU) and adk_voc_convtr_wgrad (IN_ACT_LEAKY)
static int convtr_wgrad(const std::string& f, int max_act, const float* dy, const float* x, float* dw, float* db, void* workspace,
                        int n_items, int c_in, int t, int c_out, int kernel, int stride, int act, float alpha, void* stream) {
    ConvTrWGrad c;
    long long floats = 0, bytes = 0;
    int rc = convtr_wgrad_plan(f, n_items, c_in, t, c_out, kernel, stride, act, max_act, alpha, c, floats, bytes);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/x/dw/db/workspace", !dw || !workspace || (n_items > 0 && (!dy || !x)), {dy, x, dw, db, workspace});
    if (rc != ADK_OK) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(ADK_ERR_ARG, f + ": workspace must be 8-byte aligned");
    c.dy = dy; c.x = x; c.ws = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dw));
    WGRAD_LAUNCH(convtr_wgrad_kernel, c, c_in, (unsigned)((c.nn + DW_BN - 1) / DW_BN), c.slices, s);
    ADK_HIP_CHECK(hipGetLastError());
    launch_wgrad_fold(c.ws, dw, nullptr, (int)c_in, c.nn, c.slices, s);
    ADK_HIP_CHECK(hipGetLastError());
    if (db) {
        double* slab = reinterpret_cast<double*>(c.ws + floats);
        hipLaunchKernelGGL(convtr_bias_partial_kernel, dim3(c.chunks, c_out), dim3(RED_THREADS), 0, s, dy, slab, (int)c_out, c.ts,
                           (int)((long long)n_items * c.ts), c.chunk_len);
        ADK_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(convtr_bias_fold_kernel, dim3((c_out + RED_THREADS - 1) / RED_THREADS), dim3(RED_THREADS), 0, s, slab, db,
                           (int)c_out, c.chunks);
        ADK_HIP_CHECK(hipGetLastError());
    }
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_convtr_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t stride,
                                     int64_t* workspace_bytes, int32_t* slices) {
    ConvTrWGrad g;
    long long floats = 0, bytes = 0;
    const int rc = convtr_wgrad_plan("adk_convtr_wgrad_plan", n_items, c_in, t, c_out, kernel, stride, IN_ACT_NONE, IN_ACT_NONE, 0.f, g,
                                     floats, bytes);
    if (rc != ADK_OK) return rc;
    if (workspace_bytes) *workspace_bytes = bytes;
    if (slices) *slices = g.slices;
    return ADK_OK;
}

extern "C" int adk_convtr_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in,
                                int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream) {
    return convtr_wgrad("adk_convtr_wgrad", IN_ACT_ELU, dy, x, dw, db, workspace, n_items, c_in, t, c_out, kernel, stride, act, alpha, stream);
}
extern "C" int adk_voc_convtr_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items,
                                    int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha,
                                    void* stream) {
    return convtr_wgrad("adk_voc_convtr_wgrad", IN_ACT_LEAKY, dy, x, dw, db, workspace, n_items, c_in, t, c_out, kernel, stride, act, alpha,
                        stream);
}
