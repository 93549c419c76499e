// Residual-VQ codebook re-estimation: the training branch of VectorQuantize.forward (layers/vq_module.py:74-80) for every stage of
// one ResidualVQ.forward (vq_module.py:119-134), from the latents and the codes the search emitted for them.
//   cluster_size <- decay*cluster_size + (1-decay)*count            embed_avg <- decay*embed_avg + (1-decay)*sum_{rows with code k} r_s
//   S = sum_k cluster_size      smoothed_k = (cluster_size_k + eps) / (S + size*eps) * S      embed[:,k] = embed_avg[:,k] / smoothed_k
// r_s is the residual entering stage s, rebuilt with the search kernels' own step (rvq_residual_step) from the OLD codes of every
// stage: the reference looks `quantize` up before a stage writes its new embed, so one pass over the pre-update table gives every
// stage's statistics.
//
// Bitwise reproducible and independent of how rows map to workgroups: the per-code sums run over the code's rows in ASCENDING ROW
// ORDER in f64 (a stable counting sort by code gives every (stage, code) its rows in that order -- integer arithmetic only, so the
// chunking of the sort cannot change it), S is an f64 sum in a fixed order that depends on `size` alone, and the EMA and the
// quotients are f32 with explicit round-to-nearest operations, nothing contracted.  No floating-point atomics anywhere.
//
// Launches (docs/design/rvq_ema.md):
//   T  transpose   old embed [n_q][dim][size] -> row-major twin in the workspace (coalesced gathers for A)
//   A  residuals   one wave per row: residual of every stage -> workspace; integer histogram per (chunk of rows, stage, code)
//   S1 scan        per (stage, code): exclusive prefix over the chunks, the code's count
//   S2 stage       per stage: exclusive prefix over the codes (segment starts), cluster_size EMA, S, smoothed
//   B  rank        one wave per (chunk, stage): each row's slot in its code's segment, in row order
//   C  sums        one wave per (stage, code): f64 sum of its rows' residuals, rounded once to f32, row-major
//   D  write       per (stage, 64 codes): embed_avg EMA, embed, enorm, codebook -- transposed through LDS, coalesced both ways
#include "adk_common.h"
#include <atomic>

namespace adk {

constexpr int EMA_DIM_MAX = 128;
constexpr int EMA_NQ_MAX = 16;
constexpr int EMA_THREADS = 256;
constexpr int EMA_WAVES = EMA_THREADS / 64;
constexpr int EMA_MAX_CHUNKS = 256;                    // chunks of rows of the counting sort; more rows -> longer chunks (waves loop)
constexpr int EMA_CHUNK_ROWS = 16;                     // rows per chunk until EMA_MAX_CHUNKS is reached (4 rows per wave of launch A)
constexpr int EMA_TILE = 64;                           // codes per workgroup of the transposing launches
constexpr long long EMA_MAX_BINS = 1LL << 28;          // n_q*size: keeps every code and tile index of the launches inside an int
constexpr int EMA_FLAG_BAD_INDEX = 1;                  // adk_debug_flags bit 0, as adk_rvq_stats sets it

static std::atomic<int> g_ema_chunk_rows{0};           // adk_set_option("rvq_ema_chunk_rows"): 0 = EMA_CHUNK_ROWS; results do not depend on it (tests)

int rvq_ema_set_option(const char* name, int value) {
    if (strcmp(name, "rvq_ema_chunk_rows")) return 1;
    if (value < 0) return -1;
    g_ema_chunk_rows = value;
    return 0;
}

static int ema_chunk_rows(int n_rows) {
    const int want = g_ema_chunk_rows.load();
    const long long floor_rows = ((long long)n_rows + EMA_MAX_CHUNKS - 1) / EMA_MAX_CHUNKS;
    return (int)std::max<long long>(want > 0 ? want : EMA_CHUNK_ROWS, floor_rows);
}

// ---- workspace layout (every region 256-byte aligned) ----
struct EmaLayout {
    size_t old_rows, resid, sumf, table, count, seg, smoothed, order, bytes;
};
static EmaLayout ema_layout(long long n_rows, int n_q, int dim, int size) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t bins = (size_t)n_q * size;
    const size_t chunks = (size_t)std::min<long long>(n_rows, EMA_MAX_CHUNKS);     // the most any chunking uses
    EmaLayout l;
    size_t o = 0;
    l.old_rows = o; o = up(o + bins * dim * sizeof(float));                  // [n_q*size][dim]      old codes, row-major
    l.resid = o;    o = up(o + (size_t)n_q * n_rows * dim * sizeof(float)); // [n_q][n_rows][dim]   residual entering each stage
    l.sumf = o;     o = up(o + bins * dim * sizeof(float));                  // [n_q*size][dim]      per-code sums, rounded to f32
    l.table = o;    o = up(o + chunks * bins * sizeof(int));                 // [chunks][n_q*size]   histogram, then prefix over chunks, then cursor
    l.count = o;    o = up(o + bins * sizeof(int));                          // [n_q*size]           rows of each code
    l.seg = o;      o = up(o + bins * sizeof(int));                          // [n_q*size]           first slot of each code within its stage
    l.smoothed = o; o = up(o + bins * sizeof(float));                        // [n_q*size]           Laplace-smoothed cluster size
    l.order = o;    o = up(o + (size_t)n_q * n_rows * sizeof(int));          // [n_q][n_rows]        rows sorted by code, ascending within a code
    l.bytes = o;
    return l;
}

// T: [dim][size] -> [size][dim] for one stage and one tile of 64 codes
__global__ __launch_bounds__(EMA_THREADS) void ema_transpose_kernel(const float* __restrict__ embed, float* __restrict__ rows, int dim, int size) {
    __shared__ float tile[EMA_TILE][EMA_DIM_MAX + 1];
    const int s = blockIdx.y, k0 = blockIdx.x * EMA_TILE, tid = threadIdx.x;
    const float* e = embed + (size_t)s * dim * size;
    for (int i = tid; i < dim * EMA_TILE; i += EMA_THREADS) {
        const int d = i / EMA_TILE, kk = i % EMA_TILE;
        if (k0 + kk < size) tile[kk][d] = e[(size_t)d * size + k0 + kk];
    }
    __syncthreads();
    for (int i = tid; i < dim * EMA_TILE; i += EMA_THREADS) {
        const int kk = i / dim, d = i % dim;
        if (k0 + kk < size) rows[((size_t)s * size + k0 + kk) * dim + d] = tile[kk][d];
    }
}

// A: one wave per row, as rvq_stats_kernel: lane l holds components l and l + 64, lane s reads stage s's index, all n_q code rows
// are loaded before the chain.  Writes the residual ENTERING each stage and counts the code in the chunk's histogram row.
__global__ __launch_bounds__(EMA_THREADS) void ema_residual_kernel(const float* __restrict__ z, const float* __restrict__ codebook,
                                                                   const long long* __restrict__ idx, int n_rows, int n_q, int dim, int size,
                                                                   int chunk_rows, float* __restrict__ resid, int* __restrict__ table,
                                                                   int* __restrict__ err) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const size_t bins = (size_t)n_q * size;
    const bool has0 = lane < dim, has1 = lane + 64 < dim;
    const bool stage_lane = lane < n_q;
    const long long base = (long long)size * lane;
    const long long row_lim = (long long)(chunk + 1) * chunk_rows;
    const long long row_end = row_lim < n_rows ? row_lim : n_rows;
    for (long long row = (long long)chunk * chunk_rows + wave; row < row_end; row += EMA_WAVES) {
        long long my = stage_lane ? idx[(size_t)lane * n_rows + row] : 0;
        const bool ok = stage_lane && my >= base && my < base + size;
        if (stage_lane && !ok) {                       // not a code of its stage: flag it, read the stage's code 0, count nothing
            atomicOr(err, EMA_FLAG_BAD_INDEX);
            my = base;
        }
        float r0 = has0 ? z[(size_t)row * dim + lane] : 0.f;
        float r1 = has1 ? z[(size_t)row * dim + lane + 64] : 0.f;
        float q0[EMA_NQ_MAX], q1[EMA_NQ_MAX];
#pragma unroll
        for (int s = 0; s < EMA_NQ_MAX; ++s) {
            q0[s] = q1[s] = 0.f;
            if (s < n_q) {
                const float* q = codebook + (size_t)__shfl(my, s, 64) * dim;
                if (has0) q0[s] = q[lane];
                if (has1) q1[s] = q[lane + 64];
            }
        }
        if (ok) atomicAdd(&table[(size_t)chunk * bins + my], 1);
#pragma unroll
        for (int s = 0; s < EMA_NQ_MAX; ++s) {
            if (s < n_q) {
                float* out = resid + ((size_t)s * n_rows + row) * dim;
                if (has0) out[lane] = r0;
                if (has1) out[lane + 64] = r1;
                rvq_residual_step(r0, q0[s]);
                rvq_residual_step(r1, q1[s]);
            }
        }
    }
}

// S1: one thread per (stage, code): exclusive prefix of its histogram column over the chunks, in place; the total is its count.
__global__ __launch_bounds__(EMA_THREADS) void ema_scan_chunks_kernel(int* __restrict__ table, int* __restrict__ count, int chunks, int bins) {
    const int b = blockIdx.x * EMA_THREADS + threadIdx.x;
    if (b >= bins) return;
    int run = 0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) {
        const int v = table[(size_t)c * bins + b];
        table[(size_t)c * bins + b] = run;
        run += v;
    }
    count[b] = run;
}

// S2: one workgroup per stage.  Thread t owns the contiguous codes [t*per, (t+1)*per): segment starts (exclusive prefix of the counts),
// the cluster_size EMA, S = sum of the new cluster sizes in f64 (codes in order within a thread, threads in order), smoothed.
__global__ __launch_bounds__(EMA_THREADS) void ema_stage_kernel(const int* __restrict__ count, int* __restrict__ seg, float* __restrict__ cluster_size,
                                                                float* __restrict__ smoothed, int size, float decay, float one_minus_decay,
                                                                float eps, float size_eps) {
    __shared__ long long cnt_part[EMA_THREADS];
    __shared__ double sum_part[EMA_THREADS];
    __shared__ double total;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int per = (size + EMA_THREADS - 1) / EMA_THREADS;
    const int k0 = (int)((long long)tid * per < size ? (long long)tid * per : size), k1 = (int)((long long)k0 + per < size ? (long long)k0 + per : size);
    const size_t off = (size_t)s * size;
    long long c = 0;
    double sum = 0.0;
    for (int k = k0; k < k1; ++k) {
        const int n = count[off + k];
        c += n;
        const float cs = __fadd_rn(__fmul_rn(decay, cluster_size[off + k]), __fmul_rn(one_minus_decay, (float)n));
        cluster_size[off + k] = cs;
        sum += (double)cs;
    }
    cnt_part[tid] = c;
    sum_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        double t = 0.0;
        for (int i = 0; i < EMA_THREADS; ++i) {
            const long long v = cnt_part[i];
            cnt_part[i] = run;
            run += v;
            t += sum_part[i];
        }
        total = t;
    }
    __syncthreads();
    const float S = (float)total;
    const float den = __fadd_rn(S, size_eps);
    long long run = cnt_part[tid];
    for (int k = k0; k < k1; ++k) {
        seg[off + k] = (int)run;
        run += count[off + k];
        smoothed[off + k] = __fmul_rn(__fdiv_rn(__fadd_rn(cluster_size[off + k], eps), den), S);
    }
}

// B: one wave per (chunk, stage), 64 rows at a time in row order.  A row's slot = segment start of its code + rows of that code in
// earlier chunks (the prefix S1 left in the table) + rows of that code earlier in this chunk (the table entry doubles as the
// running cursor: this wave is its only user).  Rows whose index is outside the stage get no slot.
__global__ __launch_bounds__(64) void ema_rank_kernel(const long long* __restrict__ idx, int n_rows, int size, int chunk_rows, int bins,
                                                      int* table, const int* __restrict__ seg, int* __restrict__ order) {
    const int chunk = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const long long base = (long long)size * s;
    const long long row0 = (long long)chunk * chunk_rows;
    const long long row_end = row0 + chunk_rows < n_rows ? row0 + chunk_rows : n_rows;
    int* cursor = table + (size_t)chunk * bins + (size_t)s * size;
    for (long long b0 = row0; b0 < row_end; b0 += 64) {
        const long long row = b0 + lane;
        int k = -1;
        if (row < row_end) {
            const long long v = idx[(size_t)s * n_rows + row];
            if (v >= base && v < base + size) k = (int)(v - base);
        }
        int before = 0;
        bool later = false;
        for (int j = 0; j < 64; ++j) {
            const int kj = __shfl(k, j, 64);
            before += (j < lane && kj == k) ? 1 : 0;
            later |= (j > lane && kj == k);
        }
        const int cur = k >= 0 ? cursor[k] : 0;
        __syncthreads();                               // every lane has read its cursor before any lane moves one
        if (k >= 0) {
            const int slot = cur + before;
            order[(size_t)s * n_rows + seg[(size_t)s * size + k] + slot] = (int)row;
            if (!later) cursor[k] = slot + 1;
        }
        __syncthreads();                               // the next 64 rows read the cursors this batch wrote
    }
}

// C: one wave per (stage, code): the f64 sum of the residuals of its rows, in ascending row order, rounded once to f32.
__global__ __launch_bounds__(EMA_THREADS) void ema_sum_kernel(const float* __restrict__ resid, const int* __restrict__ order,
                                                              const int* __restrict__ count, const int* __restrict__ seg, int n_rows,
                                                              int dim, int size, int bins, float* __restrict__ sumf) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * EMA_WAVES + (threadIdx.x >> 6);
    if (b >= bins) return;
    const int s = b / size;
    const int n = count[b];
    const int* rows = order + (size_t)s * n_rows + seg[b];
    const float* r = resid + (size_t)s * n_rows * dim;
    const bool has0 = lane < dim, has1 = lane + 64 < dim;
    double a0 = 0.0, a1 = 0.0;
    int i = 0;
    for (; i + 4 <= n; i += 4) {                       // four rows in flight, added in order
        float v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* p = r + (size_t)rows[i + u] * dim;
            v0[u] = has0 ? p[lane] : 0.f;
            v1[u] = has1 ? p[lane + 64] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a0 += (double)v0[u]; a1 += (double)v1[u]; }
    }
    for (; i < n; ++i) {
        const float* p = r + (size_t)rows[i] * dim;
        if (has0) a0 += (double)p[lane];
        if (has1) a1 += (double)p[lane + 64];
    }
    if (has0) sumf[(size_t)b * dim + lane] = (float)a0;
    if (has1) sumf[(size_t)b * dim + lane + 64] = (float)a1;
}

// D: one workgroup per (stage, 64 codes).  The sums come in row-major (coalesced), go through LDS, and embed_avg / embed are read
// and written with the code index fastest (coalesced in their [dim][size] layout); the new codes go back through LDS for the
// row-major twin and |e|^2.
__global__ __launch_bounds__(EMA_THREADS) void ema_write_kernel(const float* __restrict__ sumf, const float* __restrict__ smoothed,
                                                                float* __restrict__ embed_avg, float* __restrict__ embed,
                                                                float* __restrict__ enorm, float* __restrict__ codebook, int dim, int size,
                                                                float decay, float one_minus_decay) {
    __shared__ float tile[EMA_TILE][EMA_DIM_MAX + 1];
    const int s = blockIdx.y, k0 = blockIdx.x * EMA_TILE, tid = threadIdx.x;
    const size_t bin0 = (size_t)s * size + k0;
    for (int i = tid; i < dim * EMA_TILE; i += EMA_THREADS) {
        const int kk = i / dim, d = i % dim;
        if (k0 + kk < size) tile[kk][d] = sumf[(bin0 + kk) * dim + d];
    }
    __syncthreads();
    for (int i = tid; i < dim * EMA_TILE; i += EMA_THREADS) {
        const int d = i / EMA_TILE, kk = i % EMA_TILE;
        if (k0 + kk < size) {
            const size_t at = ((size_t)s * dim + d) * size + k0 + kk;
            const float ea = __fadd_rn(__fmul_rn(decay, embed_avg[at]), __fmul_rn(one_minus_decay, tile[kk][d]));
            embed_avg[at] = ea;
            const float e = __fdiv_rn(ea, smoothed[bin0 + kk]);
            embed[at] = e;
            tile[kk][d] = e;
        }
    }
    __syncthreads();
    if (codebook)
        for (int i = tid; i < dim * EMA_TILE; i += EMA_THREADS) {
            const int kk = i / dim, d = i % dim;
            if (k0 + kk < size) codebook[(bin0 + kk) * dim + d] = tile[kk][d];
        }
    if (tid < EMA_TILE && k0 + tid < size) {
        double n2 = 0.0;
        for (int d = 0; d < dim; ++d) n2 += (double)__fmul_rn(tile[tid][d], tile[tid][d]);
        enorm[bin0 + tid] = (float)n2;
    }
}

static const char* ema_check_shape(int32_t n_rows, int32_t n_q, int32_t dim, int32_t size) {
    if (n_rows <= 0) return "need n_rows > 0 (the reference's update of an empty batch divides by zero on a fresh codebook)";
    if (n_q <= 0 || n_q > EMA_NQ_MAX) return "need 0 < n_q <= 16";
    if (dim <= 0 || dim > EMA_DIM_MAX) return "need 0 < dim <= 128";
    if (size <= 0 || (long long)n_q * size > EMA_MAX_BINS) return "need size > 0 and n_q*size <= 2^28";
    return nullptr;
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_rvq_ema_workspace_bytes(int32_t n_rows, int32_t n_q, int32_t dim, int32_t size) {
    if (const char* why = ema_check_shape(n_rows, n_q, dim, size)) return fail(ADK_ERR_ARG, std::string("adk_rvq_ema_workspace_bytes: ") + why);
    return (int64_t)ema_layout(n_rows, n_q, dim, size).bytes;
}

extern "C" int adk_rvq_ema_update(const float* z, const int64_t* idx, int32_t n_rows, int32_t n_q, int32_t dim, int32_t size,
                                  double decay, double eps, float* embed, float* enorm, float* codebook, float* cluster_size,
                                  float* embed_avg, void* workspace, void* stream) {
    if (!z || !idx || !embed || !enorm || !cluster_size || !embed_avg || !workspace) return fail(ADK_ERR_ARG, "adk_rvq_ema_update: null pointer");
    if (const char* why = ema_check_shape(n_rows, n_q, dim, size)) return fail(ADK_ERR_ARG, std::string("adk_rvq_ema_update: ") + why);
    if (!(decay >= 0.0 && decay < 1.0)) return fail(ADK_ERR_ARG, "adk_rvq_ema_update: need 0 <= decay < 1");
    if (!(eps > 0.0)) return fail(ADK_ERR_ARG, "adk_rvq_ema_update: need eps > 0");
    if ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(workspace)) & 7)
        return fail(ADK_ERR_ARG, "adk_rvq_ema_update: idx/workspace must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(embed) | reinterpret_cast<uintptr_t>(enorm) |
         reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(cluster_size) | reinterpret_cast<uintptr_t>(embed_avg)) & 3)
        return fail(ADK_ERR_ARG, "adk_rvq_ema_update: z/embed/enorm/codebook/cluster_size/embed_avg must be 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(embed));
    const EmaLayout l = ema_layout(n_rows, n_q, dim, size);
    char* ws = static_cast<char*>(workspace);
    float* old_rows = reinterpret_cast<float*>(ws + l.old_rows);
    float* resid = reinterpret_cast<float*>(ws + l.resid);
    float* sumf = reinterpret_cast<float*>(ws + l.sumf);
    int* table = reinterpret_cast<int*>(ws + l.table);
    int* count = reinterpret_cast<int*>(ws + l.count);
    int* seg = reinterpret_cast<int*>(ws + l.seg);
    float* smoothed = reinterpret_cast<float*>(ws + l.smoothed);
    int* order = reinterpret_cast<int*>(ws + l.order);
    const int bins = n_q * size;
    const int chunk_rows = ema_chunk_rows(n_rows);
    const int chunks = (int)(((long long)n_rows + chunk_rows - 1) / chunk_rows);       // <= EMA_MAX_CHUNKS, <= n_rows: inside the layout's table
    const int tiles = (size + EMA_TILE - 1) / EMA_TILE;
    const float fdecay = (float)decay, fomd = (float)(1.0 - decay);                     // what torch makes of the Python scalars
    const auto* ix = reinterpret_cast<const long long*>(idx);

    ADK_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)chunks * bins * sizeof(int), st));
    hipLaunchKernelGGL(ema_transpose_kernel, dim3(tiles, n_q), dim3(EMA_THREADS), 0, st, embed, old_rows, dim, size);
    hipLaunchKernelGGL(ema_residual_kernel, dim3(chunks), dim3(EMA_THREADS), 0, st, z, old_rows, ix, n_rows, n_q, dim, size, chunk_rows,
                       resid, table, flags_word());
    hipLaunchKernelGGL(ema_scan_chunks_kernel, dim3((bins + EMA_THREADS - 1) / EMA_THREADS), dim3(EMA_THREADS), 0, st, table, count, chunks, bins);
    hipLaunchKernelGGL(ema_stage_kernel, dim3(n_q), dim3(EMA_THREADS), 0, st, count, seg, cluster_size, smoothed, size, fdecay, fomd,
                       (float)eps, (float)((double)size * eps));
    hipLaunchKernelGGL(ema_rank_kernel, dim3(chunks, n_q), dim3(64), 0, st, ix, n_rows, size, chunk_rows, bins, table, seg, order);
    hipLaunchKernelGGL(ema_sum_kernel, dim3((bins + EMA_WAVES - 1) / EMA_WAVES), dim3(EMA_THREADS), 0, st, resid, order, count, seg, n_rows,
                       dim, size, bins, sumf);
    hipLaunchKernelGGL(ema_write_kernel, dim3(tiles, n_q), dim3(EMA_THREADS), 0, st, sumf, smoothed, embed_avg, embed, enorm, codebook, dim,
                       size, fdecay, fomd);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
