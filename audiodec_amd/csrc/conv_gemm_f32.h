// The exact-f32 implicit-GEMM core of the discriminator convs, forward and backward to the input (disc.hip's disc_gemm_kernel and
// disc_gemm_grad_kernel, univ_disc.hip's conv2d_gemm_kernel and conv2d_gemm_grad_kernel), and what else the two families share:
// the argument structs' pointers, the activation and its mask, the phase split of a strided backward, and the check of act / impl.
//   Y[m][n] = bias[m] + sum_kk W[kk][m] X[kk][n]   on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a k-ordered fmaf chain,
//   no split precision), then LeakyReLU -- or another last step, the Epi parameter (dec_grad.hip's residual add and a'(x) factor).
// Workgroup tile BM x BN x 16 of 4 waves, WM x WN waves each holding TM x TN tiles of 32 x 32.  The 16-deep K slice of W
// (pre-transposed at load to [kk][m], coalesced along m) and of the implicit X are staged in LDS; the next slice is loaded into
// registers while the current one is multiplied.  A thread stages one fixed column of X over the whole K loop.
//
// What a conv is comes from Src, a per-file struct built from the kernel's arguments:
//   int k_extent(), m_extent()       GEMM K, and the M of this grid slice (one group)
//   long long n_cols()               GEMM N
//   const float* weights()           W of this grid slice, [kk][m]
//   void column(long long col)       fix this thread's staged column (may be >= n_cols())
//   float tap(int kk)                X[kk][that column]; 0 outside the input, past K, or for an invalid column
//   float* out(long long n)          where (m = 0, column n < n_cols()) lands
//   long long out_stride()           distance between output channels
//   int bias_index(int m)            index of row m's bias
#pragma once
#include "adk_common.h"

namespace adk {

constexpr int CG_THREADS = 256;                     // also the block size of every other kernel of disc.hip and univ_disc.hip
constexpr int CG_KT = 16;                           // K depth of one LDS slice
constexpr int CG_ACT_NONE = 0, CG_ACT_LEAKY = 2;
constexpr int CG_IMPL_DIRECT = 1, CG_IMPL_GEMM = 2;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float cg_act(float v, int act, float slope) {
    return (act == CG_ACT_LEAKY && v < 0.f) ? v * slope : v;
}

// A conv's INPUT activation in the training kernels (dec_grad.hip, enc_grad.hip, dec_wgrad.hip) and its derivative: none,
// ELU(alpha) (the inference kernels' ELU for alpha = 1) or LeakyReLU(alpha), whose derivative at 0 is the slope, as torch's is.
constexpr int IN_ACT_NONE = 0, IN_ACT_ELU = 1, IN_ACT_LEAKY = 2;
__device__ __forceinline__ float in_act(float v, int act, float alpha) {
    if (act == IN_ACT_NONE || v > 0.f) return v;
    return act == IN_ACT_ELU ? alpha * expm1_neg(v) : alpha * v;
}
__device__ __forceinline__ float in_dact(float v, int act, float alpha) {
    if (act == IN_ACT_NONE || v > 0.f) return 1.f;
    return act == IN_ACT_ELU ? alpha * (expm1_neg(v) + 1.f) : alpha;
}

// The pointers of a conv's argument struct, which is one of these and the family's geometry.
struct CgForwardPtrs {
    const float* x;
    const float* w;
    const float* bias;                              // [c_out] or null
    float* y;
};
struct CgBackwardPtrs {
    const float* dy;
    const float* y;                                 // of dy's shape: the forward's output (read when act is leaky)
    const float* w;
    float* dx;
};

// dz at idx of a layer's output: dy through the activation's mask, taken from the saved post-activation output y (y > 0 exactly
// where the pre-activation is, for slope >= 0).
__device__ __forceinline__ float cg_dz(const float* dy, const float* y, int act, float slope, long long idx) {
    const float v = dy[idx];
    return (act == CG_ACT_LEAKY && !(y[idx] > 0.f)) ? v * slope : v;
}

// One axis of a strided backward's phase split (kernel k, stride s, phase r = (index + pad) % s): taps r, r + s, ... < k of
// phase r; the taps of the phases before r; the first input index of phase r; how many of n input indices first, first + s, ...
// there are.
__host__ __device__ inline int phase_taps(int k, int s, int r) { return r < k ? (k - r + s - 1) / s : 0; }
__host__ __device__ inline int phase_taps_before(int k, int s, int r) { return (k / s) * r + (k % s < r ? k % s : r); }
__host__ __device__ inline int phase_first(int pad, int s, int r) { return ((r - pad) % s + s) % s; }
__host__ __device__ inline int phase_count(int n, int s, int first) { return first < n ? (n - first + s - 1) / s : 0; }

// The check of act (cg_check_act: also disc_wgrad.hip's, which has no impl) and of impl that both conv families' entry points make, f the
// entry point's name; `masked`: also slope >= 0 for a leaky layer (the backward, whose mask is cg_dz's).
static inline int cg_check_act(const std::string& f, int act, float slope, bool masked) {
    if (act != CG_ACT_NONE && act != CG_ACT_LEAKY) return fail(ADK_ERR_ARG, f + ": act must be 0 (none) or 2 (leaky)");
    if (masked && act == CG_ACT_LEAKY && !(slope >= 0.f))
        return fail(ADK_ERR_ARG, f + ": the mask is taken from the output, which needs slope >= 0");
    return ADK_OK;
}
static inline int cg_check_act_impl(const std::string& f, int act, float slope, int impl, bool masked) {
    if (const int rc = cg_check_act(f, act, slope, masked)) return rc;
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, f + ": impl must be 1 (direct) or 2 (gemm)");
    return ADK_OK;
}

// The epilogue's last step: what is stored at dst for an accumulator with its bias added.  The discriminators' is the
// activation; dec_grad.hip's add a residual or multiply by a saved input's activation derivative (Epi of conv_gemm_f32).
struct CgActStore {
    __device__ __forceinline__ void operator()(float* dst, float v, int act, float slope) const { *dst = cg_act(v, act, slope); }
};

template <int WM, int WN, int TM, int TN, class Src, class Epi = CgActStore>
__device__ __forceinline__ void conv_gemm_f32(Src& src, const float* __restrict__ bias, int act, float slope, const Epi epi = Epi()) {
    static_assert(WM * WN * 64 == CG_THREADS, "four waves");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    static_assert(CG_THREADS % BN == 0 && (BM * CG_KT) % CG_THREADS == 0, "tile shape");
    constexpr int LDA = (BM % 64 == 0) ? BM + 32 : BM;        // lanes 32..63 read the next K row: put it 32 banks over
    constexpr int LDB = (BN % 64 == 0) ? BN + 32 : BN;
    constexpr int A_PER = BM * CG_KT / CG_THREADS;
    constexpr int B_PER = BN * CG_KT / CG_THREADS;
    constexpr int B_KSTEP = CG_THREADS / BN;
    __shared__ float As[CG_KT * LDA];
    __shared__ float Bs[CG_KT * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int m0 = blockIdx.y * BM;
    const long long n0 = (long long)blockIdx.x * BN;
    const int kg = src.k_extent(), mg = src.m_extent();

    const int bn = tid % BN, bk0 = tid / BN;
    src.column(n0 + bn);
    const float* __restrict__ wg = src.weights();

    float ra[A_PER], rb[B_PER];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * CG_THREADS;
            const int k = k0 + e / BM, m = m0 + e % BM;
            ra[i] = (k < kg && m < mg) ? wg[(size_t)k * mg + m] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) rb[i] = src.tap(k0 + bk0 + i * B_KSTEP);
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * CG_THREADS;
            As[(e / BM) * LDA + e % BM] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) Bs[(bk0 + i * B_KSTEP) * LDB + bn] = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int n_kt = (kg + CG_KT - 1) / CG_KT;
    load(0);
    const int arow = wm * TM * 32 + (lane & 31), brow = wn * TN * 32 + (lane & 31), kh = lane >> 5;
    for (int kt = 0; kt < n_kt; ++kt) {
        store();
        __syncthreads();
        if (kt + 1 < n_kt) load((kt + 1) * CG_KT);
#pragma unroll
        for (int kk = 0; kk < CG_KT; kk += 2) {
            float av[TM], bv[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) av[a] = As[(kk + kh) * LDA + arow + a * 32];
#pragma unroll
            for (int b = 0; b < TN; ++b) bv[b] = Bs[(kk + kh) * LDB + brow + b * 32];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: C/D map col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long long ldy = src.out_stride();
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const long long n = n0 + wn * TN * 32 + b * 32 + (lane & 31);
        if (n >= src.n_cols()) continue;
        float* yb = src.out(n);
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * TM * 32 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < mg) {
                    const float bv = bias ? bias[src.bias_index(m)] : 0.f;
                    epi(yb + (long long)m * ldy, acc[a][b][r] + bv, act, slope);
                }
            }
    }
}

}  // namespace adk
