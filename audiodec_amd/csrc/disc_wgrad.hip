// The HiFi-GAN discriminator's training half: the gradient of the strided, zero-padded, grouped (N, C, H, P) conv that disc.hip's
// adk_disc_conv computes, with respect to its weight and bias -- what the discriminator's own update needs
// (trainer/trainerGAN.py:256-294).  Exact f32 on v_mfma_f32_32x32x2_f32; every output element is written once by one accumulator,
// nothing is added atomically, and every split of a sum is a function of the shape alone: bitwise reproducible.
//
// x [n_items][c_in][h_in][P] is the layer's input, y and dy [n_items][c_out][h_out][P] its saved output (after the activation) and
// the upstream gradient; h_out = (h_in + 2 pad - k) / s + 1, g = o / (C_out/G), ci < C_in/G:
//   dz[i][o][h'][j] = dy[i][o][h'][j] (act == leaky ? (y[i][o][h'][j] > 0 ? 1 : slope) : 1)         (cg_dz's convention, also at y == 0)
//   dW[o][ci][t]    = sum_{i,h',j} dz[i][o][h'][j] x[i][g C_in/G + ci][h' s - pad + t][j]              (x outside [0, h_in) is 0)
//   db[o]           = sum_{i,h',j} dz[i][o][h'][j]
//
//   disc_wgrad_kernel:  wgrad_gemm.h's core, one GEMM per group: M = C_out/G, N = (C_in/G) k + 1 (n = ci k + t; the last column's
//                       operand is 1: db, left out when db is not asked for), reduction over rho = (i h_out + h') P + j, along which
//                       dy and y are contiguous inside an item.  The mask is applied to the A operand when the registers are stored
//                       to LDS (two loads per element, as DiscGradSrc::tap; no elementwise pass of its own).  A B element is an
//                       operand when 0 <= h' s - pad + t < h_in: a two-sided test, unlike the causal kernel's.  Rows of x the
//                       forward never reached (the tail when h_in + 2 pad - k is no multiple of s) are never addressed.
//                       blockIdx.z = g S + slice (disc_wgrad_plan); the workspace is [slice][g C_out/G + m][n]: the layout of dW
//                       itself ([co][ci][k]), which wgrad_gemm.h's fold then writes.
#include "wgrad_gemm.h"

namespace adk {

struct DiscWGrad {
    int n_items, c_in, h_in, period, c_out, groups, ksz, stride, pad, h_out, act;
    float slope;
    int cin_g, cout_g;                              // channels of one group
    int hp_in, hp_out;                              // h_in * period, h_out * period: positions per channel
    int ck;                                         // cin_g * ksz: columns 0 .. ck - 1 are dW's, column ck is db's
    int nc_live;                                    // columns computed: ck + 1, or ck when db is not asked for
    int red;                                        // n_items * hp_out: the reduction length
    int steps_per, slices;                          // 32-deep steps of one slice, and S
    const float* dy; const float* y;                // y is dy when there is no mask to take (never a null load)
    const float* x; float* ws;                      // ws [slices][c_out][ck + 1]
};                                                  // the grid's z is groups * slices

constexpr int DW_NO_TAP = -0x40000000;              // t - pad of a column that reads no x: its row test fails for every h'

// wgrad_gemm.h's Stage of the discriminator's conv: A is dz (dy through y's mask), B is x at tap (ci, t), or 1 in db's column.
template <int BM, int BN>
struct DiscWGradStage {
    static constexpr int A_PER = BM / WG_ROWS, B_PER = BN / WG_ROWS;
    const int kr = threadIdx.x % WG_KT, row0 = threadIdx.x / WG_KT;    // this thread's reduction offset in a step, and its first row
    const int m0, row_g;                                        // the tile's first row in the group, the group's first dy row
    const bool leaky;
    int xoff[B_PER], trow[B_PER];                               // per column: x offset of tap (ci, t) in an item at h' = 0, j = 0; its row t - pad
    unsigned bias_col = 0;                                      // bit i: this thread's column i is db's
    float ra[A_PER], ry[A_PER], rb[B_PER];
    unsigned amask = 0, bmask = 0;
    bool live = false;

    __device__ __forceinline__ DiscWGradStage(const DiscWGrad& c, int grp, int m0_, int n0)
        : m0(m0_), row_g(grp * c.cout_g), leaky(c.act == CG_ACT_LEAKY) {
        const int ch_g = grp * c.cin_g;                         // the group's first x channel
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int n = n0 + row0 + i * WG_ROWS;
            const bool tap = n < c.ck;                          // the bias column and columns past it read no x
            const int ci = n / c.ksz, tr = n - ci * c.ksz - c.pad;
            xoff[i] = tap ? (ch_g + ci) * c.hp_in + tr * c.period : 0;
            trow[i] = tap ? tr : DW_NO_TAP;
            bias_col |= (n == c.ck && n < c.nc_live) ? 1u << i : 0u;
        }
    }
    __device__ __forceinline__ void prepare(float*, int) {}
    // clamped address: element 0 of the tensor (a step exists only when the operands do)
    __device__ __forceinline__ void load(const DiscWGrad& c, int step) {
        const int rho = step * WG_KT + kr;
        live = rho < c.red;
        const int item = live ? rho / c.hp_out : 0, rem = live ? rho - item * c.hp_out : 0;
        const int ho = rem / c.period, j = rem - ho * c.period;
        const long long ybase = (long long)item * c.c_out * c.hp_out + rem;
        const float* __restrict__ dyb = c.dy + ybase;
        const float* __restrict__ yb = c.y + ybase;
        const float* __restrict__ xb = c.x + (long long)item * c.c_in * c.hp_in;
        const int hb = ho * c.stride, q = hb * c.period + j;
        amask = bmask = 0;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int m = m0 + row0 + i * WG_ROWS;
            const bool ok = live && m < c.cout_g;
            const long long off = ok ? (long long)(row_g + m) * c.hp_out : -(long long)rem;      // clamped: the item's element 0
            ra[i] = dyb[off];
            ry[i] = yb[off];
            amask |= ok ? 1u << i : 0u;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const bool ok = live && (unsigned)(hb + trow[i]) < (unsigned)c.h_in;
            rb[i] = xb[ok ? xoff[i] + q : 0];
            bmask |= ok ? 1u << i : 0u;
        }
    }
    __device__ __forceinline__ void store(const DiscWGrad& c, float* As, int LDA, float* Bs, int LDB) const {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const float dz = (leaky && !(ry[i] > 0.f)) ? ra[i] * c.slope : ra[i];
            As[kr * LDA + row0 + i * WG_ROWS] = (amask >> i & 1) ? dz : 0.f;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const float one = (live && (bias_col >> i & 1)) ? 1.f : 0.f;
            Bs[kr * LDB + row0 + i * WG_ROWS] = (bmask >> i & 1) ? rb[i] : one;
        }
    }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void disc_wgrad_kernel(DiscWGrad c) {
    const int grp = blockIdx.z / c.slices, slice = blockIdx.z - grp * c.slices;
    DiscWGradStage<WM * TM * 32, WN * TN * 32> stage(c, grp, blockIdx.y * (WM * TM * 32), blockIdx.x * (WN * TN * 32));
    wgrad_gemm<WM, WN, TM, TN>(stage, c, c.red, c.steps_per, slice, c.cout_g, c.nc_live,
                               c.ws + ((size_t)slice * c.c_out + grp * c.cout_g) * (c.ck + 1), c.ck + 1);
}

// ---- host ----
// disc_geometry's conditions on a layer (disc.hip), under this entry point's name, then the 32-bit limits of the kernel's
// indices and the slice rule: wgrad_gemm.h's wgrad_slices with the tiles of all groups.
static int disc_wgrad_plan(const std::string& f, int n_items, int c_in, int h_in, int period, int c_out, int groups, int kernel,
                           int stride, int pad, DiscWGrad& g, long long& ws_bytes) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || period <= 0 || c_out <= 0 || groups <= 0 || kernel <= 0 || stride <= 0 || pad < 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, h_in, period, c_out, groups, kernel, stride > 0, pad >= 0");
    if (c_in % groups || c_out % groups) return fail(ADK_ERR_ARG, f + ": groups must divide c_in and c_out");
    const long long span = (long long)h_in + 2LL * pad - kernel;
    if (span < 0) return fail(ADK_ERR_ARG, f + ": kernel longer than the padded input");
    const long long h_out = span / stride + 1, hp_in = (long long)h_in * period, hp_out = h_out * period;
    const int cin_g = c_in / groups, cout_g = c_out / groups;
    const long long red = (long long)n_items * hp_out, ck = (long long)cin_g * kernel;
    // c_in * hp_in bounds every x offset inside an item; (h_in + 2 pad) * period the row part h' s P + j of one before the tap's
    if ((long long)h_in + 2LL * pad >= (1LL << 30) || (long long)c_in * kernel >= (1LL << 30) || c_in * hp_in >= (1LL << 31) ||
        ((long long)h_in + 2LL * pad) * period >= (1LL << 31) || red >= (1LL << 31) - WG_KT || c_out * (ck + 1) >= (1LL << 31) ||
        (cout_g + 31) / 32 > 65535)
        return fail(ADK_ERR_ARG, f + ": layer too large");
    long long steps_per = 1, slices = 1;
    wgrad_slices(wgrad_tiles(groups, cout_g, ck + 1), (red + WG_KT - 1) / WG_KT, steps_per, slices);
    if (groups * slices > 65535) return fail(ADK_ERR_ARG, f + ": layer too large (groups * slices is the grid's z)");
    g.n_items = n_items; g.c_in = c_in; g.h_in = h_in; g.period = period; g.c_out = c_out; g.groups = groups; g.ksz = kernel;
    g.stride = stride; g.pad = pad; g.h_out = (int)h_out; g.cin_g = cin_g; g.cout_g = cout_g; g.hp_in = (int)hp_in;
    g.hp_out = (int)hp_out; g.ck = (int)ck; g.nc_live = (int)ck + 1; g.red = (int)red; g.steps_per = (int)steps_per;
    g.slices = (int)slices;
    ws_bytes = slices * c_out * (ck + 1) * 4;
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_disc_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t h_in, int32_t period, int32_t c_out, int32_t groups,
                                        int32_t kernel, int32_t stride, int32_t pad, int64_t* workspace_bytes, int32_t* slices) {
    DiscWGrad g;
    long long bytes = 0;
    const int rc = disc_wgrad_plan("adk_disc_conv_wgrad_plan", n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad, g, bytes);
    if (rc != ADK_OK) return rc;
    if (workspace_bytes) *workspace_bytes = bytes;
    if (slices) *slices = g.slices;
    return ADK_OK;
}

extern "C" int adk_disc_conv_wgrad(const float* dy, const float* y, const float* x, float* dw, float* db, void* workspace,
                                   int32_t n_items, int32_t c_in, int32_t h_in, int32_t period, int32_t c_out, int32_t groups,
                                   int32_t kernel, int32_t stride, int32_t pad, int32_t act, float slope, void* stream) {
    const std::string f = "adk_disc_conv_wgrad";
    DiscWGrad c;
    long long bytes = 0;
    int rc = disc_wgrad_plan(f, n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad, c, bytes);
    if (rc != ADK_OK) return rc;
    rc = cg_check_act(f, act, slope, true);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "dy/y/x/dw/db/workspace", !dw || !workspace || (n_items > 0 && (!dy || !x || (act == CG_ACT_LEAKY && !y))),
                        {dy, y, x, dw, db, workspace});
    if (rc != ADK_OK) return rc;
    c.act = act; c.slope = slope;
    c.dy = dy; c.y = act == CG_ACT_LEAKY ? y : dy; c.x = x; c.ws = static_cast<float*>(workspace);
    c.nc_live = db ? c.ck + 1 : c.ck;                          // without db its column is not computed
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dw));
    WGRAD_LAUNCH(disc_wgrad_kernel, c, c.cout_g, (unsigned)((c.nc_live + 127) / 128), (unsigned)(groups * c.slices), s);
    ADK_HIP_CHECK(hipGetLastError());
    launch_wgrad_fold(c.ws, dw, db, (int)c_out, c.ck, c.slices, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
