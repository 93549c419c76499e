// The second launch of every weight gradient (wgrad_gemm.h): one thread per (m, n) adds the S partial tiles ws[slice][m][n] (rows
// of ck + 1 floats) in ascending slice order in f64, rounds once and stores dw[m ck + n] or, for the last column n = ck, db[m]
// (db null: that column is neither read nor written).  The library's one copy, for enc_grad.hip, dec_wgrad.hip and disc_wgrad.hip.
#include "wgrad_gemm.h"

namespace adk {

__global__ __launch_bounds__(CG_THREADS) void wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ dw,
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

void launch_wgrad_fold(const float* ws, float* dw, float* db, int rows, int ck, int slices, hipStream_t s) {
    const long long total = (long long)rows * (db ? ck + 1 : ck);
    hipLaunchKernelGGL(wgrad_fold_kernel, dim3((unsigned)((total + CG_THREADS - 1) / CG_THREADS)), dim3(CG_THREADS), 0, s, ws, dw, db,
                       rows, ck, slices);
}

}  // namespace adk
