// The reproducible f64 sum every loss entry point ends in (mel.hip, stft_loss.hip, disc.hip): per-lane f64 sums, the 64-lane
// butterfly, waves in index order, one f64 partial per workgroup in a caller-supplied slab (the workgroup count is a function of
// the shape only), and a one-wave finalize launch that folds the slab in a fixed order into the running totals.  No float
// atomics: the sum is bitwise the same run to run.
#pragma once
#include "adk_common.h"

namespace adk {

constexpr int RED_THREADS = 256;                       // the workgroup workgroup_partials serves
constexpr int RED_WAVES = RED_THREADS / 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sums of a WAVES-wave workgroup in wave order into partial[NS * blockIdx.x ..].
template <int NS, int WAVES = RED_WAVES>
__device__ __forceinline__ void workgroup_partials(double (&acc)[NS], double* __restrict__ partial) {
    __shared__ double wsum[WAVES][NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double t = wave_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = wsum[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) t += wsum[w][threadIdx.x];
        partial[NS * (size_t)blockIdx.x + threadIdx.x] = t;
    }
}

// One wave: folds the slab into sums (workgroups in a fixed order) and adds count.  NS = 3: sc = sqrt(s0) / sqrt(s1) and
// mag = s2 / count from the totals; NS = 1: mag = s0 / count.  NaN on an empty total.
template <int NS>
__global__ __launch_bounds__(64) void distance_finalize_kernel(const double* __restrict__ partial, int n_wg, long long n_values,
                                                               double* __restrict__ sums, long long* __restrict__ count,
                                                               float* __restrict__ sc, float* __restrict__ mag) {
    const int lane = threadIdx.x;
    double t[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double v = 0.0;
        for (int b = lane; b < n_wg; b += 64) v += partial[NS * (size_t)b + j];
        t[j] = wave_sum(v);
    }
    if (lane == 0) {
        const long long n = count[0] + n_values;
        count[0] = n;
#pragma unroll
        for (int j = 0; j < NS; ++j) { t[j] += sums[j]; sums[j] = t[j]; }
        const float nan = __builtin_nanf("");
        if (sc) sc[0] = n > 0 ? (float)(sqrt(t[0]) / sqrt(t[NS > 1 ? 1 : 0])) : nan;
        if (mag) mag[0] = n > 0 ? (float)(t[NS - 1] / (double)n) : nan;
    }
}

// The finalize launch after the n_wg partials of NS sums each (n_wg = 0: only the totals and results).
template <int NS>
static inline void launch_distance_finalize(const void* workspace, int n_wg, long long n_values, double* sums, int64_t* count,
                                            float* sc, float* mag, hipStream_t s) {
    hipLaunchKernelGGL(distance_finalize_kernel<NS>, dim3(1), dim3(64), 0, s, static_cast<const double*>(workspace), n_wg, n_values,
                       sums, reinterpret_cast<long long*>(count), sc, mag);
}

// Workgroups of a slab launch: one per item up to cap, at least one.
static inline int capped_workgroups(long long items, int cap) {
    return (int)std::min<long long>(std::max<long long>(items, 1), cap);
}

// The accumulator, slab and result pointers every distance entry point takes.
static inline int check_accumulators(const char* fn, const void* sums, const void* count, const void* workspace,
                                     bool need_workspace, const void* r0, const void* r1) {
    const std::string f(fn);
    if (!sums || !count) return fail(ADK_ERR_ARG, f + ": null accumulator pointer");
    if (need_workspace && !workspace) return fail(ADK_ERR_ARG, f + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(workspace)) & 7)
        return fail(ADK_ERR_ARG, f + ": sums/count/workspace must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(r1)) & 3)
        return fail(ADK_ERR_ARG, f + ": result pointers must be 4-byte aligned");
    return ADK_OK;
}

}  // namespace adk
