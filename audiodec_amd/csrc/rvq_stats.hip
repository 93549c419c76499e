// Residual-VQ statistics of emitted codes: the per-stage commitment loss and code histogram of VectorQuantize.forward /
// ResidualVQ.forward (layers/vq_module.py:61-88, 119-134) in eval mode, from the latents and the indices adk_rvq_encode wrote.
//   loss_s       = mse(q_s, r_s)                      q_s = codebook row idx[s][row], r_s = residual entering stage s
//   perplexity_s = exp(-sum_k p_k log(p_k + 1e-10))   p_k = count_k / rows, in f32 as torch.mean of the one-hot gives it
// The residual chain is rebuilt with the search kernels' own step (rvq_residual_step, adk_common.h), so r_s is the residual the
// search saw, bit for bit.  Results are bitwise reproducible: the squared errors are summed in f64 in a fixed order (in rows order
// per lane, lanes by a butterfly, waves of a workgroup in index order, workgroups by the finalize launch in a fixed
// order: per-workgroup partial slabs, no float atomics); the histogram is integer (LDS per workgroup, then global integer adds).
#include "adk_common.h"

namespace adk {

constexpr int STATS_DIM_MAX = 128;
constexpr int STATS_NQ_MAX = 16;
constexpr int STATS_THREADS = 256;                     // 4 waves, one row per wave at a time
constexpr int STATS_WAVES = STATS_THREADS / 64;
constexpr int STATS_MAX_WG = 1024;                     // one row per wave up to 4096 rows; beyond, the waves loop over rows
constexpr int STATS_HIST_LDS_BINS = 16384;             // n_q*size up to this is histogrammed in LDS (64 KB: 16 x 1024); larger: global adds
constexpr int STATS_FLAG_BAD_INDEX = 1;                // adk_debug_flags bit 0, as adk_rvq_lookup sets it

static int stats_workgroups(long long n_rows) {
    const long long g = (n_rows + STATS_WAVES - 1) / STATS_WAVES;
    return (int)std::min<long long>(std::max<long long>(g, 1), STATS_MAX_WG);
}

// One wave per row: lane l holds components l and l + 64.  Every load of a row is issued before its residual chain: lane s
// reads stage s's index, then all n_q code rows land in registers (one coalesced 256-byte read per 64 components each) --
// two dependent memory round trips per row, whatever n_q (the indices do not depend on the residuals).  Then per stage,
// in registers: (q - r)^2 into the lane's f64 sum of that stage, the residual step.  Lane s counts stage s's code.
template <bool LDS_HIST>
__global__ __launch_bounds__(STATS_THREADS) void rvq_stats_kernel(const float* __restrict__ z, const float* __restrict__ codebook,
                                                                  const long long* __restrict__ idx, int n_rows, int n_q, int dim, int size,
                                                                  unsigned long long* __restrict__ counts, double* __restrict__ partial,
                                                                  long long* __restrict__ rows, int* __restrict__ err) {
    extern __shared__ int hist[];                      // LDS_HIST: n_q*size bins, global index order
    __shared__ double wsum[STATS_WAVES][STATS_NQ_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bins = n_q * size;
    if (LDS_HIST) {
        for (int b = tid; b < bins; b += STATS_THREADS) hist[b] = 0;
        __syncthreads();
    }
    const bool has0 = lane < dim, has1 = lane + 64 < dim;
    const bool stage_lane = lane < n_q;
    const long long base = (long long)size * lane;     // first index of stage `lane`
    double esum[STATS_NQ_MAX];
#pragma unroll
    for (int s = 0; s < STATS_NQ_MAX; ++s) esum[s] = 0.0;
    for (int row = blockIdx.x * STATS_WAVES + wave; row < n_rows; row += gridDim.x * STATS_WAVES) {
        long long my = stage_lane ? idx[(size_t)lane * n_rows + row] : 0;
        const bool ok = stage_lane && my >= base && my < base + size;
        if (stage_lane && !ok) {                       // not a code of its stage: flag it, read the stage's code 0, count nothing
            atomicOr(err, STATS_FLAG_BAD_INDEX);
            my = base;
        }
        float r0 = has0 ? z[(size_t)row * dim + lane] : 0.f;
        float r1 = has1 ? z[(size_t)row * dim + lane + 64] : 0.f;
        float q0[STATS_NQ_MAX], q1[STATS_NQ_MAX];
#pragma unroll
        for (int s = 0; s < STATS_NQ_MAX; ++s) {
            q0[s] = q1[s] = 0.f;
            if (s < n_q) {
                const float* q = codebook + (size_t)__shfl(my, s, 64) * dim;
                if (has0) q0[s] = q[lane];
                if (has1) q1[s] = q[lane + 64];
            }
        }
        if (ok) {
            if (LDS_HIST) atomicAdd(&hist[my], 1);
            else atomicAdd(&counts[my], 1ull);
        }
#pragma unroll
        for (int s = 0; s < STATS_NQ_MAX; ++s) {
            if (s < n_q) {
                const float d0 = __fsub_rn(q0[s], r0), d1 = __fsub_rn(q1[s], r1);     // f32 difference, f32 square: nothing contracted
                esum[s] += (double)__fmul_rn(d0, d0) + (double)__fmul_rn(d1, d1);
                rvq_residual_step(r0, q0[s]);
                rvq_residual_step(r1, q1[s]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < STATS_NQ_MAX; ++s) {
        if (s < n_q) {
            double e = esum[s];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off, 64);
            if (lane == 0) wsum[wave][s] = e;
        }
    }
    __syncthreads();
    if (LDS_HIST)
        for (int b = tid; b < bins; b += STATS_THREADS) {
            const int h = hist[b];
            if (h) atomicAdd(&counts[b], (unsigned long long)h);
        }
    if (tid < n_q) {
        double t = 0.0;
        for (int w = 0; w < STATS_WAVES; ++w) t += wsum[w][tid];
        partial[(size_t)tid * gridDim.x + blockIdx.x] = t;            // slab [n_q][workgroups]
    }
    if (blockIdx.x == 0 && tid == 0) rows[0] += n_rows;
}

// One workgroup per stage: folds the stage's slab into sse (workgroups in a fixed order) and writes vqloss / perplexity from
// the accumulated totals (the row count was folded by the launch before).
__global__ __launch_bounds__(STATS_THREADS) void rvq_stats_finalize_kernel(const double* __restrict__ partial, int n_wg, int dim, int size,
                                                                          const unsigned long long* __restrict__ counts,
                                                                          double* __restrict__ sse, const long long* __restrict__ rows,
                                                                          float* __restrict__ vqloss, float* __restrict__ perplexity) {
    __shared__ double red[2][STATS_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long total = rows[0];
    const float n = (float)total;
    double t = 0.0, h = 0.0;
    for (int b = tid; b < n_wg; b += STATS_THREADS) t += partial[(size_t)s * n_wg + b];
    if (perplexity)
        for (int k = tid; k < size; k += STATS_THREADS) {
            const unsigned long long c = counts[(size_t)s * size + k];
            if (c) {                                   // p = 0 adds 0 * log(1e-10)
                const float p = __fdiv_rn((float)c, n);
                h += (double)p * log((double)__fadd_rn(p, 1e-10f));
            }
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        t += __shfl_xor(t, off, 64);
        h += __shfl_xor(h, off, 64);
    }
    if (lane == 0) { red[0][wave] = t; red[1][wave] = h; }
    __syncthreads();
    if (tid == 0) {
        double ts = 0.0, hs = 0.0;
        for (int w = 0; w < STATS_WAVES; ++w) { ts += red[0][w]; hs += red[1][w]; }
        const double acc = sse[s] + ts;
        sse[s] = acc;
        if (vqloss) vqloss[s] = total > 0 ? (float)(acc / ((double)total * (double)dim)) : __builtin_nanf("");
        if (perplexity) perplexity[s] = total > 0 ? (float)exp(-hs) : __builtin_nanf("");
    }
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_rvq_stats_workspace_bytes(int32_t n_rows, int32_t n_q) {
    if (n_rows < 0 || n_q <= 0 || n_q > STATS_NQ_MAX) return fail(ADK_ERR_ARG, "adk_rvq_stats_workspace_bytes: need n_rows >= 0, 0 < n_q <= 16");
    if (n_rows == 0) return 0;
    return (int64_t)stats_workgroups(n_rows) * n_q * (int64_t)sizeof(double);
}

extern "C" int adk_rvq_stats(const float* z, const float* codebook, const int64_t* idx, int32_t n_rows, int32_t n_q, int32_t dim,
                             int32_t size, int64_t* counts, double* sse, int64_t* rows, void* workspace, float* vqloss,
                             float* perplexity, void* stream) {
    if (!counts || !sse || !rows) return fail(ADK_ERR_ARG, "adk_rvq_stats: null accumulator pointer");
    if (n_rows > 0 && (!z || !codebook || !idx || !workspace)) return fail(ADK_ERR_ARG, "adk_rvq_stats: null pointer");
    if (n_rows < 0 || n_q <= 0 || n_q > STATS_NQ_MAX) return fail(ADK_ERR_ARG, "adk_rvq_stats: need n_rows >= 0, 0 < n_q <= 16");
    if (dim <= 0 || dim > STATS_DIM_MAX) return fail(ADK_ERR_ARG, "adk_rvq_stats: need 0 < dim <= 128");
    if (size <= 0 || (long long)n_q * size > 0x7fffffffLL || (long long)n_q * size * dim > 0x7fffffffffffLL)
        return fail(ADK_ERR_ARG, "adk_rvq_stats: need size > 0 and n_q*size < 2^31");
    if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(sse) | reinterpret_cast<uintptr_t>(rows) |
         reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(workspace)) & 7)
        return fail(ADK_ERR_ARG, "adk_rvq_stats: idx/counts/sse/rows/workspace must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(vqloss) |
         reinterpret_cast<uintptr_t>(perplexity)) & 3)
        return fail(ADK_ERR_ARG, "adk_rvq_stats: z/codebook/vqloss/perplexity must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sse));
    const int n_wg = n_rows > 0 ? stats_workgroups(n_rows) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n_rows > 0) {
        auto* cnt = reinterpret_cast<unsigned long long*>(counts);
        const auto* ix = reinterpret_cast<const long long*>(idx);
        const int bins = n_q * size;
        if (bins <= STATS_HIST_LDS_BINS) {
            static bool attr_set[kMaxDevices] = {};
            bool& set = attr_set[current_device()];
            if (!set) {
                ADK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(rvq_stats_kernel<true>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, STATS_HIST_LDS_BINS * (int)sizeof(int)));
                set = true;
            }
            hipLaunchKernelGGL(rvq_stats_kernel<true>, dim3(n_wg), dim3(STATS_THREADS), (size_t)bins * sizeof(int), s,
                               z, codebook, ix, n_rows, n_q, dim, size, cnt, partial, reinterpret_cast<long long*>(rows), flags_word());
        } else {
            hipLaunchKernelGGL(rvq_stats_kernel<false>, dim3(n_wg), dim3(STATS_THREADS), 0, s,
                               z, codebook, ix, n_rows, n_q, dim, size, cnt, partial, reinterpret_cast<long long*>(rows), flags_word());
        }
        ADK_HIP_CHECK(hipGetLastError());
    } else if (!vqloss && !perplexity) {
        return ADK_OK;                                 // nothing to fold, nothing asked for
    }
    hipLaunchKernelGGL(rvq_stats_finalize_kernel, dim3(n_q), dim3(STATS_THREADS), 0, s, partial, n_wg, dim, size,
                       reinterpret_cast<const unsigned long long*>(counts), sse, reinterpret_cast<const long long*>(rows), vqloss, perplexity);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
