// The weight-gradient GEMM core of the three training kernels -- enc_grad.hip's wgrad_kernel (causal conv), dec_wgrad.hip's
// convtr_wgrad_kernel (CausalConvTranspose1d) and disc_wgrad.hip's disc_wgrad_kernel (the discriminator's (N, C, H, P) conv) --
// and what else they share: the depth of a reduction step, the rule that cuts the reduction into slices, the tile dispatch, the
// check of an input activation, and the launch that folds the slices' f32 partial tiles (wgrad_fold.hip).
//   D[m][n] = sum_rho A[rho][m] B[rho][n]   on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate), rho in this workgroup's slice
// Workgroup tile BM x BN x 32 of 4 waves, WM x WN waves each holding TM x TN tiles of 32 x 32.  Both operands are activations,
// contiguous along rho in memory: a 32-deep step of each is staged TRANSPOSED in LDS, As[rho][m] and Bs[rho][n], rows padded to
// 33 mod 64 floats (the transposed stores of 32 lanes along rho hit 32 banks, and lanes 32..63 read the next row 33 banks over).
// The next step's loads are issued into registers while the current step is multiplied.  The summation order of an element is
// this file's loop and nothing else: steps ascending, kk ascending inside a step, one accumulator; the slices in wgrad_fold.hip.
//
// What a conv is comes from Stage, a per-file struct that is a local of the kernel, built from (args, group, m0, n0): it holds
// this thread's row and column tables, its staging registers and their masks.  args is the kernel's argument struct, which the
// core hands to load and store: a Stage that keeps a reference to it costs convtr_wgrad_kernel 24 to 28 VGPRs and its 32-row tile
// the third wave per SIMD (docs/design/encoder_grad.md).
//   void prepare(float* Bs, int n)                          once, before the first step, by every thread (n floats of Bs; may barrier)
//   void load(const Args& args, int step)                   issue the loads of rows [32 step, 32 step + 32) of A and B into registers:
//                                                           unconditional, from clamped addresses; what is no operand is masked
//   void store(const Args& args, float* As, int LDA, float* Bs, int LDB)
//                                                           write what load() fetched, masked and activated, to As[rho][m] / Bs[rho][n]:
//                                                           every slot of both tiles that prepare() did not settle, every step
// wgrad_gemm(stage, args, red, steps_per, slice, m_live, n_live, ws_tile_base, ws_row_floats): the reduction length, the steps of a
// slice and this workgroup's slice; the rows and columns of the tile grid that exist; where (m = 0, n = 0) of this slice (and
// group) lands in the workspace, and the floats of a workspace row.
//
//   wgrad_slices:        S is a function of the shape only: with `tiles` output tiles (wgrad_tiles) and n_steps 32-deep steps,
//                        S0 = min(ceil(512 / tiles), max(1, n_steps / 4)), a slice is ceil(n_steps / S0) steps and S the slices
//                        that many steps make (so no slice is empty; the last one may be short).
//   launch_wgrad_fold:   wgrad_fold_kernel, one thread per (m, n): the S partials ws[slice][m][n] (rows of ck + 1 floats) in
//                        ascending slice order in f64, rounded once, stored as dw[m ck + n] or, for the last column n = ck, db[m]
//                        (db null: that column is neither read nor written).  No float atomics: bitwise the same run to run.
#pragma once
#include "conv_gemm_f32.h"

namespace adk {

constexpr int WG_KT = 32;                           // reduction depth of one LDS slice of the weight gradient
constexpr int WG_ROWS = CG_THREADS / WG_KT;         // tile rows (or columns) one pass of the 256 threads stages
constexpr int WG_TARGET_WGS = 512;                  // workgroups a weight-gradient launch aims at (two per CU of 256)
constexpr int WG_MIN_STEPS = 4;                     // a slice is at least this many 32-deep steps (when there are that many)

template <int WM, int WN, int TM, int TN, class Stage, class Args>
__device__ __forceinline__ void wgrad_gemm(Stage& stage, const Args& args, int red, int steps_per, int slice, int m_live, int n_live,
                                           float* __restrict__ ws_tile_base, int ws_row_floats) {
    static_assert(WM * WN * 64 == CG_THREADS, "four waves");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    static_assert(BM % WG_ROWS == 0 && BN % WG_ROWS == 0, "tile shape");
    constexpr int LDA = (BM % 64 == 0) ? BM + 33 : BM + 1;
    constexpr int LDB = (BN % 64 == 0) ? BN + 33 : BN + 1;
    __shared__ float As[WG_KT * LDA];
    __shared__ float Bs[WG_KT * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    stage.prepare(Bs, WG_KT * LDB);

    const int n_steps = (red + WG_KT - 1) / WG_KT;
    const int s0 = slice * steps_per, s1 = min(n_steps, s0 + steps_per);
    const int arow = wm * TM * 32 + (lane & 31), brow = wn * TN * 32 + (lane & 31), kh = lane >> 5;
    if (s0 < s1) stage.load(args, s0);
    for (int st = s0; st < s1; ++st) {
        stage.store(args, As, LDA, Bs, LDB);
        __syncthreads();
        if (st + 1 < s1) stage.load(args, st + 1);
#pragma unroll
        for (int kk = 0; kk < WG_KT; kk += 2) {
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

    // C/D map col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); the partial tile goes to ws_tile_base[m][n], the
    // slice's (and group's) part of the workspace, m < m_live and n < n_live only
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int n = n0 + wn * TN * 32 + b * 32 + (lane & 31);
        if (n >= n_live) continue;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * TM * 32 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < m_live) ws_tile_base[(size_t)m * ws_row_floats + n] = acc[a][b][r];
            }
    }
}

// ---- host ----
// The tile follows M: 128 x 128 from M >= 128, 64 x 128 from M >= 64, else 32 x 128.  wgrad_tiles: the output tiles of `groups`
// GEMMs of m rows and n_cols columns, what wgrad_slices is given.
static inline long long wgrad_tiles(long long groups, int m, long long n_cols) {
    const int bm = m >= 128 ? 128 : m >= 64 ? 64 : 32;
    return groups * ((m + bm - 1) / bm) * ((n_cols + 127) / 128);
}

static inline void wgrad_slices(long long tiles, long long n_steps, long long& steps_per, long long& slices) {
    const long long want = std::max<long long>(1, (WG_TARGET_WGS + tiles - 1) / tiles);
    const long long s0 = std::max<long long>(1, std::min<long long>(want, n_steps / WG_MIN_STEPS));
    steps_per = std::max<long long>(1, (n_steps + s0 - 1) / s0);
    slices = std::max<long long>(1, (n_steps + steps_per - 1) / steps_per);
}

// kernel<WM, WN, TM, TN>(c) over nx column tiles, the row tiles of m and a grid z of nz
#define WGRAD_LAUNCH(kernel, c, m, nx, nz, s)                                                                                \
    do {                                                                                                                     \
        if ((m) >= 128) hipLaunchKernelGGL((kernel<2, 2, 2, 2>), dim3(nx, ((m) + 127) / 128, nz), dim3(CG_THREADS), 0, s, c); \
        else if ((m) >= 64) hipLaunchKernelGGL((kernel<2, 2, 1, 2>), dim3(nx, ((m) + 63) / 64, nz), dim3(CG_THREADS), 0, s, c); \
        else hipLaunchKernelGGL((kernel<1, 4, 1, 1>), dim3(nx, ((m) + 31) / 32, nz), dim3(CG_THREADS), 0, s, c);             \
    } while (0)

// The check of a conv's input activation (conv_gemm_f32.h's in_act); max_act is the largest act the entry point f takes.
static inline int wgrad_check_in_act(const std::string& f, int act, int max_act, float alpha) {
    if (act < IN_ACT_NONE || act > max_act)
        return fail(ADK_ERR_ARG, f + (max_act == IN_ACT_ELU ? ": act must be 0 (none) or 1 (ELU)" : ": act must be 0 (none), 1 (ELU) or 2 (LeakyReLU)"));
    if (act != IN_ACT_NONE && !(alpha == alpha)) return fail(ADK_ERR_ARG, f + ": alpha is NaN");
    return ADK_OK;
}

// The fold launch after the GEMM's (wgrad_fold.hip): rows x (ck [+ 1 with db]) outputs.
void launch_wgrad_fold(const float* ws, float* dw, float* db, int rows, int ck, int slices, hipStream_t s);

}  // namespace adk
