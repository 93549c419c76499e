// What the weight-gradient GEMMs share (enc_grad.hip's wgrad_kernel, dec_wgrad.hip's convtr_wgrad_kernel): the depth of a
// reduction step, the rule that cuts the reduction into slices, and the launch that folds the slices' f32 partial tiles.
//   wgrad_slices:        S is a function of the shape only: with `tiles` output tiles and n_steps 32-deep steps,
//                        S0 = min(ceil(512 / tiles), max(1, n_steps / 4)), a slice is ceil(n_steps / S0) steps and S the slices
//                        that many steps make (so no slice is empty; the last one may be short).
//   wgrad_fold_kernel:   one thread per (m, n): the S partials ws[slice][m][n] (rows of ck + 1 floats) in ascending slice order in
//                        f64, rounded once, stored as dw[m ck + n] or, for the last column n = ck, db[m] (db null: that column is
//                        neither read nor written).  No float atomics: bitwise the same run to run.
#pragma once
#include "conv_gemm_f32.h"

namespace adk {

constexpr int WG_KT = 32;                           // reduction depth of one LDS slice of the weight gradient
constexpr int WG_TARGET_WGS = 512;                  // workgroups a weight-gradient launch aims at (two per CU of 256)
constexpr int WG_MIN_STEPS = 4;                     // a slice is at least this many 32-deep steps (when there are that many)

static inline void wgrad_slices(long long tiles, long long n_steps, long long& steps_per, long long& slices) {
    const long long want = std::max<long long>(1, (WG_TARGET_WGS + tiles - 1) / tiles);
    const long long s0 = std::max<long long>(1, std::min<long long>(want, n_steps / WG_MIN_STEPS));
    steps_per = std::max<long long>(1, (n_steps + s0 - 1) / s0);
    slices = std::max<long long>(1, (n_steps + steps_per - 1) / steps_per);
}

static __global__ __launch_bounds__(CG_THREADS) void wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                       float* __restrict__ db, int c_out, int ck, int slices) {
    const int nc = ck + 1, nc_live = db ? nc : ck;
    const long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
    if (o >= (long long)c_out * nc_live) return;
    const int m = (int)(o / nc_live), n = (int)(o - (long long)m * nc_live);
    const size_t total = (size_t)c_out * nc;
    const float* __restrict__ p = ws + (size_t)m * nc + n;
    double s = 0.0;
    int z = 0;
    for (; z + 8 <= slices; z += 8) {                           // eight loads in flight, added in ascending order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(z + j) * total];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (double)v[j];
    }
    for (; z < slices; ++z) s += (double)p[(size_t)z * total];
    if (n < ck) dw[(size_t)m * ck + n] = (float)s;
    else db[m] = (float)s;
}

// The fold launch after the GEMM's: rows x (ck [+ 1 with db]) outputs.
static inline void launch_wgrad_fold(const float* ws, float* dw, float* db, int rows, int ck, int slices, hipStream_t s) {
    const long long total = (long long)rows * (db ? ck + 1 : ck);
    hipLaunchKernelGGL(wgrad_fold_kernel, dim3((unsigned)((total + CG_THREADS - 1) / CG_THREADS)), dim3(CG_THREADS), 0, s, ws, dw, db,
                       rows, ck, slices);
}

}  // namespace adk
