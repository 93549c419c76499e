// conv_rk16 -- the split-f16 conv for WIDE groups (>= 128 input channels per group) when a call brings SEVERAL steps per stream and the
// taps of neighbouring steps share their input rows (small dilation): rows staged once in LDS, whole tiles, no K split.
//
// The stream-K kernel (conv_mfma.hip) gathers its B operand per (column, tap): for the 256-channel K11 dilation-1 convs of the vocoder's
// first stage at 5 steps per stream that is 55 ring rows per stream and channel block of which only 15 are distinct, each 64-deep chunk
// behind a barrier -- 44 dependent iterations per tile.  Here one workgroup owns one 64 x 64 tile (one group, 64 output channels, 64
// (stream, step) columns packed densely -- a tile may begin and end inside a stream) over the WHOLE K:
//   * per 32-channel block the distinct rows of every stream the tile touches -- (taps - 1) * dilation + t_out per stream -- are staged
//     once, in the row format of conv_rl16 ([32 halfs hi][32 halfs lo][16 B pad]), double buffered: the next block's rows are requested
//     when a block begins and stored when it ends, one barrier per block.  From a shadow ring a staged piece is a 16-byte copy; from the
//     f32 ring it is act_split (conv_split16.h) -- the shadow's own bits, so the two sources cannot be told apart downstream;
//   * inside a block the loop is the one of the rows-in-LDS kernels: taps outer, B fragments by ds_read_b128 at a shifted row, A fragments
//     global -> VGPR in the adk_pack_weights_split16 order, PF steps ahead and pinned; no barrier, no global X traffic;
//   * eight waves: two per 32 x 32 quadrant, one taking the first and one the second 16 channels of every block.  One workgroup per CU
//     (240 tiles at 256 streams) is then two waves per SIMD; the pair's joined sums are added through LDS, first half + second half, a
//     fixed order;
//   * the finished tile leaves through sk_epilogue_lds (conv_sk_epilogue.h): bias, residual, activation, f32 row, shadow row -- what
//     the next conv reads is produced by the code that produces it after a stream-K launch, so a program may switch between the two
//     kernels from call to call.
// No workspace, no flag, no wait between workgroups.  Per output element the products are those of the stream-K kernel, added channel
// block by channel block instead of tap by tap and in two halves instead of one or two ranges: the results agree with it to f32
// round-off, not bit for bit; the same call is bit-reproducible.
#include "conv_sk_epilogue.h"
#include <atomic>
#include <cstdlib>

#ifndef ADK_RK16_PF11
#define ADK_RK16_PF11 3     // weight prefetch distance of the K 11 variants in 16-k steps (tuning builds: 3 or 5 -- PF + 1 divides K + 1; K 7: 3)
#endif

namespace adk {

namespace {
constexpr int kCB = 32;                          // channels per staged block
constexpr int kRS = 4 * kCB + 16;                // LDS row stride in bytes: [32 halfs hi][32 halfs lo][16 B pad]
constexpr int kNT = 512;                         // eight waves
constexpr int kRounds = 4;                       // staging rounds: 8 pieces of 16 bytes per row, 64 rows per round
constexpr int kMaxRows = 65536 / (2 * kRS);      // rows per buffer that two buffers fit in 64 KiB: 227 (< 64 * kRounds)
constexpr int kSumBytes = 2 * 4 * 64 * 64;       // the wave pairs' partial tiles: [half][quadrant][4 pieces][64 lanes] x 16 B
constexpr int kEpiBytes = kSumBytes + 64 * (64 + 4) * 4;     // ... followed by sk_epilogue_lds's tile image

struct RkArgs {
    int tiles, m_tiles, n_tiles;   // 64 x 64 tiles: all, per group along M, along N
    int nblk;                      // 32-channel blocks per tap = cin_g / 32
    int rps;                       // rows staged per stream: (taps - 1) * dilation + t_out
    int nrows;                     // rows of one LDS buffer: the most streams a tile touches x rps (<= kMaxRows)
    int ksteps;                    // 16-k steps per 32-row m-tile in the packed weights
    int mt32_per_g;
    unsigned in_bytes, w_bytes;    // buffer-descriptor extents of the input arena view / packed weights
    float inv_t_out;
    int* err;
};

std::atomic<int> g_use_rk{-1};     // adk_set_option("conv_rk16"); -1: not set yet, the environment's ADK_CONV_RK16 (default 1) decides
}  // namespace

template <int ACT, int TAPS>
__global__ __launch_bounds__(kNT, 2) void conv_rk16_kernel(ConvArgs a, RkArgs rk) {      // (512, 2): at most 128 registers per wave
    constexpr int PF = TAPS == 11 ? ADK_RK16_PF11 : 3, R = PF + 1;      // weight prefetch distance in units, slots of the fragment ring
    static_assert(PF >= 1 && PF < TAPS, "the units in flight are those of one block");
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = wave & 3, kh = wave >> 2;         // output quadrant, half of every channel block
    const int wm = quad >> 1, wn = quad & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    // XCD-contiguous tiles, M-tile fastest (as the stream-K ranges): the workgroups of one XCD share X columns and a weight panel
    const int per_xcd = (rk.tiles + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (tile >= rk.tiles) return;
    const int mt = tile % rk.m_tiles;
    const int rest = tile / rk.m_tiles;
    const int nt = rest % rk.n_tiles, g = rest / rk.n_tiles;
    const int n0 = nt * 64, m0 = mt * 64;
    const int b0 = n0 / a.t_out;                       // first stream of the tile
    const int n_last = min(n0 + 63, a.n_total - 1);
    const int rows_used = (n_last / a.t_out - b0 + 1) * rk.rps;          // <= rk.nrows (conv_rk16_eligible counts the streams)

    const __amdgpu_buffer_rsrc_t rsrc_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, rk.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wfrag), 0, rk.w_bytes, 0x00020000);
    const unsigned lane16 = (unsigned)lane * 16u;
    const unsigned bufbytes = (unsigned)rk.nrows * kRS;

    // ---- staging: thread = piece p of row (tid >> 3) + 64 k.  Row r of stream b0 + s is ring row in_row0 + r: step t, tap j reads r = t + j * dilation ----
    const int p = tid & 7;
    unsigned goff[kRounds];
    {
        const unsigned row_bytes = (unsigned)a.in_ch * 4u, ring_bytes = (unsigned)a.in_rows * row_bytes;
        const unsigned chan = (unsigned)(a.in_choff + g * a.in_gstride) * 4u + (unsigned)p * 16u;
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const int row = (tid >> 3) + 64 * k;
            goff[k] = OOB;
            if (row < rows_used) {
                const int sl = row / rk.rps, r = row - sl * rk.rps;
                int rr = a.in_row0 + r;
                if (rr >= a.in_rows) rr -= a.in_rows;
                goff[k] = (unsigned)(b0 + sl) * ring_bytes + (unsigned)rr * row_bytes + chan;
            }
        }
    }
    // shadow ring: piece p is the 8 hi halfs (even p) or the 8 lo halfs (odd p) of channels 8 (p >> 1) ..; f32 ring: 4 floats -> 4 + 4 halfs
    const unsigned ldst0 = (unsigned)(tid >> 3) * kRS + (ACT == kActPre ? (unsigned)((p & 1) * 2 * kCB + (p >> 1) * 16) : (unsigned)(8 * p));
    float4 sreg[kRounds];
    auto gload = [&](int cb) {
#pragma unroll
        for (int k = 0; k < kRounds; ++k) sreg[k] = buf_load4(rsrc_in, goff[k] != OOB ? goff[k] + (unsigned)cb * (4u * kCB) : OOB, 0);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            if (goff[k] == OOB) continue;
            unsigned char* d = xs + (unsigned)buf * bufbytes + ldst0 + (unsigned)k * (64 * kRS);
            if constexpr (ACT == kActPre) {
                *reinterpret_cast<float4*>(d) = sreg[k];
            } else {
                f16x4 hi, lo;
                act_split4<ACT>(sreg[k], a.slope, hi, lo);
                *reinterpret_cast<f16x4*>(d) = hi;
                *reinterpret_cast<f16x4*>(d + 2 * kCB) = lo;
            }
        }
    };

    // ---- weight stream: unit (block cb, tap j) of this wave is 16-k step j * cin_g / 16 + 2 cb + kh of its 32-row m-tile ----
    const unsigned wbase = (unsigned)((g * rk.mt32_per_g + mt * 2 + wm) * rk.ksteps + kh) * 2048u;
    const unsigned tap_bytes = (unsigned)rk.nblk * 2u * 2048u;       // one tap further in the packed weights
    u32x4 ah[R], al[R];

    // ---- this lane's B fragments: column n0 + 32 wn + l31 (clamped past the last column: computed, never stored), k half lh ----
    unsigned xoff;
    {
        const int nn = min(n0 + wn * 32 + l31, a.n_total - 1);
        const int b = fast_div(nn, a.t_out, rk.inv_t_out), t = nn - b * a.t_out;
        xoff = (unsigned)((b - b0) * rk.rps + t) * kRS + (unsigned)(kh * 32 + 16 * lh);
    }
    const unsigned dil_rs = (unsigned)a.dilation * kRS;

    f32x16 acc[1], accx;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; accx[e] = 0.f; }

    // ---- prologue: block 0 into buffer 0, the first PF weight units ----
    gload(0);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        ah[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16, wbase + (unsigned)i * tap_bytes, 0);
        al[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16 + 1024u, wbase + (unsigned)i * tap_bytes, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    lstore(0);
    __syncthreads();

    // ---- one channel block: straight-line code, so that the compiler's wait counts are exact -- the rows of the next block are
    // requested first and stored last (older than every weight load behind them: their wait drains nothing), a unit waits for its own
    // fragments and leaves the PF units behind it in flight.  A block is P = TAPS rounded up to whole rounds of the ring positions
    // (TAPS + 1 for K 7 and 11: one position without a unit), so that a position's ring slot is the same in every block ----
    constexpr int P = (TAPS + R - 1) / R * R;
    unsigned bufoff = 0;
    auto block = [&](int cb, auto more) {
        constexpr bool MORE = decltype(more)::value;   // another block follows
        if constexpr (MORE) gload(cb + 1);
        const unsigned wb = wbase + (unsigned)cb * 4096u;
        const unsigned char* xb = xs + bufoff + xoff;
#pragma unroll
        for (int pos = 0; pos < P; ++pos) {
            const int tpos = pos + PF, tj = tpos % P;  // the unit PF positions on: of this block, or of the next one
            if (tj < TAPS && (tpos < P || MORE)) {
                const unsigned so = wb + (tpos < P ? 0u : 4096u) + (unsigned)tj * tap_bytes;
                ah[tj % R] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16, so, 0);
                al[tj % R] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16 + 1024u, so, 0);
            }
            // keep the loads HERE (as rb_mfma): left alone the scheduler sinks them to just in front of their use
            __builtin_amdgcn_sched_barrier(0);
            if (pos < TAPS) {
                const f16x8 bh = *reinterpret_cast<const f16x8*>(xb);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(xb + 2 * kCB);
                xb += dil_rs;
                const f16x8 Ah = as_f16x8(ah[pos % R]), Al = as_f16x8(al[pos % R]);
                // per accumulator the order of the other split kernels: hi*hi | hi*lo, lo*hi
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, bh, acc[0], 0, 0, 0);
                accx = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, bl, accx, 0, 0, 0);
                accx = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, bh, accx, 0, 0, 0);
            }
        }
        if constexpr (MORE) {
            // the next block's rows go into the other buffer: every wave left it before the barrier that opened this block
            bufoff = bufbytes - bufoff;
            lstore(bufoff ? 1 : 0);
            __syncthreads();
        }
    };
    for (int cb = 0; cb + 1 < rk.nblk; ++cb) block(cb, std::true_type());
    block(rk.nblk - 1, std::false_type());

    // ---- the pair's halves: main + cross / 2048 each, then first half + second half through LDS (both waves form the same sum) ----
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][e] = join(acc[0][e], accx[e]);
    __syncthreads();                                   // every wave is done with the staged rows
    float4* S = reinterpret_cast<float4*>(xs);
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4)
        S[((kh * 4 + quad) * 4 + e4) * 64 + lane] = make_float4(acc[0][4 * e4], acc[0][4 * e4 + 1], acc[0][4 * e4 + 2], acc[0][4 * e4 + 3]);
    __syncthreads();
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
        const float4 o = S[(((kh ^ 1) * 4 + quad) * 4 + e4) * 64 + lane];
        acc[0][4 * e4] += o.x; acc[0][4 * e4 + 1] += o.y; acc[0][4 * e4 + 2] += o.z; acc[0][4 * e4 + 3] += o.w;
    }
    // both waves of a pair write the same values into the tile image; the 512 threads then take one (column, 8 channels) item each
    sk_epilogue_lds<1, 64, 64, kNT, true>(a, acc, reinterpret_cast<float*>(xs + kSumBytes), g, m0, n0, wm, wn, tid, rk.inv_t_out, rk.err);
}

// most streams a 64-column tile touches: it starts at a multiple of 64, anywhere inside a stream
static int rk_tile_streams(const ConvArgs& a) {
    const int s = (a.t_out - 1 + 63) / a.t_out + 1;
    return std::min(s, a.batch);
}

// Shape class (a function of the conv arguments alone, never of the shadow rings: both sides of a bit-for-bit comparison land on the
// same kernel): stride 1, K 7 or 11, >= 128 input channels per group in whole 64-channel blocks, whole 64-row m-tiles where the stream-K
// launch would run its 64 x 64 tiles, 8-channel groups
// that never straddle a ring row (the shadow layout, sk_epilogue_lds), every (step, tap) row used at least twice, and the rows of the
// streams of one tile within the LDS budget.
bool conv_rk16_eligible(const ConvArgs& a) {
    if (!conv_mfma_supported(a) || a.n_total < 1) return false;
    if (a.stride != 1 || a.up != 1 || (a.taps != 7 && a.taps != 11)) return false;
    if (a.cin_g < 128 || a.cin_g % 64 || a.cout_g % 64) return false;
    if (conv_sk16_pick(a) != 2) return false;          // it stands in for the 64 x 64 stream-K launch; where 128-row tiles are chosen (or a config is forced) that stands
    if ((a.in_ch % 8) || (a.in_choff % 8) || (a.in_gstride % 8) || (a.out_ch % 8) || (a.out_choff % 8) || (a.cout_real % 8)) return false;
    const long long rps = (long long)(a.taps - 1) * a.dilation + a.t_out;
    if (rps > a.in_rows || 2 * rps > (long long)a.t_out * a.taps) return false;          // (one step per stream: no row is shared)
    if (rps * rk_tile_streams(a) > kMaxRows) return false;
    return (long long)a.groups * (a.cout_g / 64) * ((a.n_total + 63) / 64) < (1ll << 28);
}

// Whole tiles pay where they fill the chip: a launch of fewer than kMinTiles tiles (three quarters of the 256 CUs; encoder block 3 at 256
// streams has 80) stays on the stream-K kernel, which cuts K to occupy the idle CUs.  Option value 2 lifts the floor (tests, A/B at few streams).
constexpr int kMinTiles = 192;

bool conv_rk16_preferred(const ConvArgs& a) {
    int on = g_use_rk.load();
    if (on < 0) {
        const char* e = getenv("ADK_CONV_RK16");
        on = e ? atoi(e) : 1;
        on = on < 0 ? 0 : (on > 2 ? 2 : on);
        g_use_rk.store(on);
    }
    if (!on || !conv_rk16_eligible(a)) return false;
    if (on == 2) return true;
    // (the x.repeat form -- every group reads the same input block, group input stride 0 -- is left to the stream-K kernel as well: the
    // parity test of the benched configuration names that launch, the first conv of a vocoder block, as a stream-K launch; docs/design/conv_rk16.md)
    if (a.groups > 1 && a.in_gstride == 0) return false;
    return (long long)a.groups * (a.cout_g / 64) * ((a.n_total + 63) / 64) >= kMinTiles;
}

void conv_rk16_set(int value) { g_use_rk.store(value <= 0 ? 0 : (value > 2 ? 2 : value)); }

int launch_conv_rk16(const ConvArgs& a, hipStream_t s) {
    if (!conv_rk16_eligible(a)) return ADK_ERR_STATE;
    RkArgs rk;
    rk.m_tiles = a.cout_g / 64;
    rk.n_tiles = (a.n_total + 63) / 64;
    rk.tiles = a.groups * rk.m_tiles * rk.n_tiles;
    rk.nblk = a.cin_g / kCB;
    rk.rps = (a.taps - 1) * a.dilation + a.t_out;
    rk.nrows = rk.rps * rk_tile_streams(a);
    rk.ksteps = a.ktot / 16;                           // (cin_g % 64 == 0: K needs no padding)
    rk.mt32_per_g = a.cout_g / 32;
    rk.in_bytes = (unsigned)((unsigned long long)a.batch * a.in_rows * a.in_ch * 4ull);                  // < 2^31: conv_mfma_supported
    rk.w_bytes = (unsigned)((unsigned long long)a.groups * rk.mt32_per_g * rk.ksteps * 2048ull);         // < 0xfff00000: the same
    rk.inv_t_out = 1.0f / (float)a.t_out;
    rk.err = conv_err_word(a);
    const size_t lds = std::max<size_t>(2 * (size_t)rk.nrows * kRS, kEpiBytes);
    const unsigned grid = (unsigned)((rk.tiles + 7) / 8 * 8);
    ConvArgs b = a;
    int act = a.act_in;
    if (a.in_sh) { b.in = a.in_sh; act = kActPre; }    // same geometry, same addressing: the pieces are staged as they are
    auto go = [&](auto act_c) -> int {
        constexpr int ACT = decltype(act_c)::value;
        if (a.taps == 7) hipLaunchKernelGGL((conv_rk16_kernel<ACT, 7>), dim3(grid), dim3(kNT), lds, s, b, rk);
        else hipLaunchKernelGGL((conv_rk16_kernel<ACT, 11>), dim3(grid), dim3(kNT), lds, s, b, rk);
        ADK_HIP_CHECK(hipGetLastError());
        return ADK_OK;
    };
    if (act == kActPre) return go(std::integral_constant<int, kActPre>());
    return with_act_in(act, "conv: unsupported input activation for the MFMA kernel", go);
}

}  // namespace adk
