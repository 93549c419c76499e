// UnivNet spectral discriminator (models/vocoder/modules/discriminator.py:451-640), exact f32: the magnitude spectrogram front
// end and the true 2-D convs over (frames, bins) planes, forward and backward to the input (the gradient of the generator-side
// GAN losses with respect to y_hat; the weights are constants).  The backward is in gather form: every output element is
// written exactly once by one thread or one accumulator, nothing is added atomically, so the gradient is bitwise reproducible.
// The period half of the UnivNet discriminator and the loss sums are disc.hip's.
//
//   spec_kernel:         torchaudio.functional.spectrogram(x, pad, window, n_fft, hop, win_length, power=1) transposed:
//                        frame f of signal s = xp[f*hop - n_fft/2 + j] (reflected at both ends of xp) * window_centred[j], where
//                        xp is x with `pad` zeros on both sides (never materialised: both paddings and the window are applied
//                        while loading, spec_load_frame); out [s][f][k] = |X_f[k]|, k <= n_fft/2, no eps clamp.  One frame per
//                        wave, the FFT of fft_wave.h; a frame's bins are one coalesced run of the output.  The load is this file's
//                        own and not stft_frame.h's: it zero-pads inside the reflect padding and writes a literal 0 outside the
//                        window.
//   spec_grad_frames_kernel: the vector-Jacobian product of spec_kernel, one frame per wave: the frame is recomputed by the same
//                        spec_load_frame, bin k gets g[k] (re, im) / |X[k]| -- (0, 0) where |X[k]| == 0, torch's abs backward
//                        (sgn(0) = 0); a frame that lies in the zero padding has only such bins -- then stft_grad.h's tail into a
//                        slab [n_signals][frames][n_fft], which stft_grad.h's gather folds per sample: sample t is position
//                        p = t + pad of the zero-padded signal of length tp = T + 2 pad; the reflect padding acts on that longer
//                        signal, so p is also reached at -p and 2 (tp - 1) - p.
//   conv2d_gemm_kernel:  x [n][c_in][H][W] -> y [n][c_out][H'][W'], kernel (kh, kw), stride (sh, sw), zero padding (ph, pw) by
//                        predicated loads, as an implicit GEMM through conv_gemm_f32.h's core:
//                          Y[m][n] = bias[m] + sum_kk W[kk][m] X[kk][n],  m < c_out,  kk = (ci*kh + th)*kw + tw,
//                          n = (item, h', w');  X[kk][n] = x[item][ci][h'*sh - ph + th][w'*sw - pw + tw]
//                        Conv2dSrc is that addressing; the wrapper builds its kk table once per workgroup in LDS.
//   conv2d_direct_kernel: one thread per output position and block of COB output channels, for the c_in = 1 first layer and
//                        the c_out = 1 output layer, where a GEMM tile would be mostly padding.  Same k order.
//   conv2d_gemm_grad_kernel: the backward
//                          dx[i][ci][h][w] = sum over co and taps (th, tw) with (h + ph - th) % sh == 0, (w + pw - tw) % sw == 0,
//                                            0 <= ho = (h + ph - th) / sh < H', 0 <= wo = (w + pw - tw) / sw < W'
//                                            of W[co][ci][th][tw] dz[i][co][ho][wo],   dz = cg_dz(dy, y)
//                        (y the layer's saved post-activation output: y > 0 exactly where its pre-activation is, for slope >= 0)
//                        as a GEMM through the same core:  M = C_in (rows of dx), N = input positions, K = (co, tap) pairs, split
//                        by PHASE (rh, rw) = ((h + ph) % sh, (w + pw) % sw): only the taps th = rh + tth sh, tw = rw + ttw sw
//                        reach such a position, so the columns are enumerated per phase, blockIdx.z = rh * sw + rw runs over the
//                        phases and the K loop of a grid slice runs over c_out * taps(rh) * taps(rw) pairs only -- no structural
//                        zero is multiplied.  W is re-packed once per layer to
//                        [phase][kk = (co * taps(rh) + tth) * taps(rw) + ttw][m]; kk -> (dy offset, tth, ttw) comes from a table in
//                        dynamic LDS built per workgroup for its phase (no division in the K loop).  A phase without taps
//                        (kernel < stride on an axis) has K = 0 and writes zeros; so do rows and columns the forward never read
//                        (every ho or wo out of range).  The activation mask is applied where a tap is staged
//                        (Conv2dGradSrc::tap).
//   conv2d_direct_grad_kernel: one thread per dx element, for the C_in = 1 first layer -- whose dx is the spectrogram's gradient
//                        -- and the C_out = 1 output layer; written for any layer shape.
#include "conv_gemm_f32.h"
#include "stft_grad.h"

namespace adk {

constexpr int UD_MAX_K = 4096;                      // GEMM: rows of the kk table (8 bytes each in LDS), either direction
constexpr int UD_SPEC_MAX_WG = 8192;

// ---- magnitude spectrogram ----
static inline long long spec_frames(int n_samples, int pad, int hop) { return 1 + ((long long)n_samples + 2LL * pad) / hop; }

// Both spectrogram kernels' arguments: stft_frame.h's (the window's placement, which the backward's shared tail reads) for
// the signal with `pad` zeros on both sides.
struct SpecArgs : StftFrameArgs {
    int pad;
    SpecArgs(int n_samples_, int pad_, int n_fft, int hop_, const float* window_, int win_length_)
        : StftFrameArgs(n_samples_, n_fft, hop_, window_, win_length_, 0.f), pad(pad_) {
        frames = spec_frames(n_samples_, pad_, hop_);
    }
};

// Frame f of signal xs into buf (NFFT floats of LDS).  Ends with a barrier.
template <int NFFT>
__device__ __forceinline__ void spec_load_frame(const float* __restrict__ xs, long long f, const SpecArgs& a, float* buf) {
    const long long tp = (long long)a.n_samples + 2LL * a.pad;            // length of the zero-padded signal
    const long long u0 = f * a.hop - NFFT / 2;
#pragma unroll 4
    for (int j = threadIdx.x; j < NFFT; j += FFT_WAVE) {
        long long u = u0 + j;
        u = u < 0 ? -u : u;                                            // reflect padding of the zero-padded signal
        u = u >= tp ? 2LL * (tp - 1) - u : u;
        const long long t = u - a.pad;                                 // zero padding
        const int jw = j - a.lpad;
        float v = 0.f;
        if (t >= 0 && t < a.n_samples && jw >= 0 && jw < a.win_length) v = __fmul_rn(xs[t], a.window[jw]);
        buf[j] = v;
    }
    __syncthreads();
}

template <int LOG2N>
__global__ __launch_bounds__(FFT_WAVE) void spec_kernel(const float* __restrict__ x, int n_signals, SpecArgs a,
                                                        float* __restrict__ out) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N;
    __shared__ float2 tw[N + 2];
    __shared__ float buf[NFFT];
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        spec_load_frame<NFFT>(x + (size_t)s * a.n_samples, f, a, buf);
        float2* z = reinterpret_cast<float2*>(buf);
        wave_fft_dif<LOG2N>(z, tw);
        float* __restrict__ o = out + (size_t)it * (N + 1);
        for (int k = lane; k <= N; k += FFT_WAVE) {
            float re, im;
            wave_fft_bin<LOG2N>(z, tw, k, re, im);
            o[k] = sqrtf(re * re + im * im);
        }
        __syncthreads();
    }
}

template <int LOG2N>
__global__ __launch_bounds__(FFT_WAVE) void spec_grad_frames_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                    int n_signals, SpecArgs a, float* __restrict__ slab) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N;
    __shared__ float2 tw[N + 2];
    __shared__ float buf[NFFT];
    __shared__ float2 keep[N + 2];
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        spec_load_frame<NFFT>(x + (size_t)s * a.n_samples, f, a, buf);
        float2* z = reinterpret_cast<float2*>(buf);
        wave_fft_dif<LOG2N>(z, tw);
        const float* __restrict__ gf = g + (size_t)it * (N + 1);
        for (int k = lane; k <= N; k += FFT_WAVE) {
            float re, im;
            wave_fft_bin<LOG2N>(z, tw, k, re, im);
            const float mag = sqrtf(re * re + im * im);                    // the forward's output
            float2 d = make_float2(0.f, 0.f);                              // |X| == 0: torch's abs backward, sgn(0) = 0
            if (mag > 0.f) {
                const float r = gf[k] / mag;
                d = make_float2(r * re, r * im);
            }
            keep[k] = d;
        }
        __syncthreads();
        frame_grad_tail<LOG2N>(a, buf, tw, keep, slab + (size_t)it * NFFT);
    }
}

static int spec_workgroups(const SpecArgs& a, int n_signals) { return (int)std::min<long long>(a.frames * n_signals, UD_SPEC_MAX_WG); }

// The checks adk_spectrogram and adk_spectrogram_grad both make.
static int check_spec_args(const std::string& f, int n_signals, int n_samples, int pad, int n_fft, int hop, const float* window,
                           int win_length) {
    const int rc = check_fft_sizes(f, n_fft, hop, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals < 0 || n_samples <= 0 || pad < 0) return fail(ADK_ERR_ARG, f + ": need n_signals >= 0, n_samples > 0, pad >= 0");
    if ((long long)n_samples + 2LL * pad <= n_fft / 2)
        return fail(ADK_ERR_ARG, f + ": reflect padding needs n_samples + 2 pad > n_fft / 2");
    if ((long long)n_samples + 2LL * pad >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": signal too long");
    if (!window) return fail(ADK_ERR_ARG, f + ": null window");
    return ADK_OK;
}

// ---- 2-D conv ----
// One layer as both directions see it; filled by conv2d_geometry.
struct Conv2dGeom {
    int n_items, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, h_out, w_out, act;
    float slope;
    long long hw_in, hw_out;                        // positions per channel
};

struct Conv2dArgs : CgForwardPtrs, Conv2dGeom {     // x [n_items][c_in][h_in][w_in] -> y [n_items][c_out][h_out][w_out]
    int kg;                                         // c_in * kh * kw: GEMM K
    long long n_cols;                               // n_items * hw_out: GEMM N
};
struct Conv2dGrad : CgBackwardPtrs, Conv2dGeom {};  // dy, y of y's shape -> dx of x's

// Rows of a kk table in LDS: K rounded up to the core's slice depth; the backward keeps one slice for a phase without taps.
__host__ __device__ inline int conv2d_table_rows(int kg) { return (kg + CG_KT - 1) / CG_KT * CG_KT; }
__host__ __device__ inline int conv2d_grad_table_rows(int kg) { return kg > 0 ? conv2d_table_rows(kg) : CG_KT; }

// What conv_gemm_f32 needs of a Conv2dArgs: both axes have taps and strides, so kk -> (input offset, th, tw) comes from ktab,
// a table in dynamic LDS (no division in the K loop), and a column gives (item base, h0, w0).
struct Conv2dSrc {
    const Conv2dArgs& c;
    const int2* ktab;                               // [conv2d_table_rows(kg)]: .x input offset of tap kk, .y th | tw << 16
    long long xbase = 0;
    int h0 = -0x40000000, w0 = -0x40000000;         // an invalid column fails every bounds test
    __device__ int k_extent() const { return c.kg; }
    __device__ int m_extent() const { return c.c_out; }
    __device__ long long n_cols() const { return c.n_cols; }
    __device__ const float* weights() const { return c.w; }
    __device__ void column(long long col) {
        if (col < c.n_cols) {
            const long long item = col / c.hw_out;
            const long long rem = col - item * c.hw_out;
            const int ho = (int)(rem / c.w_out), wo = (int)(rem - (long long)ho * c.w_out);
            h0 = ho * c.sh - c.ph;
            w0 = wo * c.sw - c.pw;
            xbase = item * c.c_in * c.hw_in + (long long)h0 * c.w_in + w0;
        }
    }
    __device__ float tap(int kk) const {
        const int2 e = ktab[kk];
        const int h = h0 + (e.y & 0xffff), w = w0 + (e.y >> 16);
        const bool ok = e.y >= 0 && (unsigned)h < (unsigned)c.h_in && (unsigned)w < (unsigned)c.w_in;
        return ok ? c.x[xbase + e.x] : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / c.hw_out, rem = n - item * c.hw_out;
        return c.y + item * c.c_out * c.hw_out + rem;
    }
    __device__ long long out_stride() const { return c.hw_out; }
    __device__ int bias_index(int m) const { return m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void conv2d_gemm_kernel(Conv2dArgs c) {
    extern __shared__ int2 ktab[];
    const int khw = c.kh * c.kw;
    for (int kk = threadIdx.x; kk < conv2d_table_rows(c.kg); kk += CG_THREADS) {
        int2 e = make_int2(0, -1);                             // past K: never loaded
        if (kk < c.kg) {
            const int ci = kk / khw, r = kk - ci * khw;
            const int th = r / c.kw, tw = r - th * c.kw;
            e = make_int2((ci * c.h_in + th) * c.w_in + tw, th | (tw << 16));
        }
        ktab[kk] = e;
    }
    __syncthreads();
    Conv2dSrc src{c, ktab};
    conv_gemm_f32<WM, WN, TM, TN>(src, c.bias, c.act, c.slope);
}

// One thread per (item, output position) and block of COB output channels (blockIdx.y); w is the reference's [c_out][kg].
template <int COB>
__global__ __launch_bounds__(CG_THREADS) void conv2d_direct_kernel(Conv2dArgs c) {
    const long long col = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
    if (col >= c.n_cols) return;
    const int co0 = blockIdx.y * COB;
    const long long item = col / c.hw_out, rem = col - item * c.hw_out;
    const int ho = (int)(rem / c.w_out), wo = (int)(rem - (long long)ho * c.w_out);
    const int h0 = ho * c.sh - c.ph, w0 = wo * c.sw - c.pw;
    const float* __restrict__ xb = c.x + item * c.c_in * c.hw_in;
    const float* __restrict__ wr = c.w + (size_t)co0 * c.kg;
    float s[COB];
#pragma unroll
    for (int q = 0; q < COB; ++q) s[q] = 0.f;
    int kk = 0;
    for (int ci = 0; ci < c.c_in; ++ci) {
        const float* xc = xb + (long long)ci * c.hw_in;
        for (int th = 0; th < c.kh; ++th) {
            const int h = h0 + th;
            for (int tw = 0; tw < c.kw; ++tw, ++kk) {
                const int w = w0 + tw;
                if ((unsigned)h < (unsigned)c.h_in && (unsigned)w < (unsigned)c.w_in) {
                    const float v = xc[(long long)h * c.w_in + w];
#pragma unroll
                    for (int q = 0; q < COB; ++q)
                        if (co0 + q < c.c_out) s[q] = fmaf(wr[(size_t)q * c.kg + kk], v, s[q]);
                }
            }
        }
    }
    float* yb = c.y + (item * c.c_out + co0) * c.hw_out + rem;
#pragma unroll
    for (int q = 0; q < COB; ++q)
        if (co0 + q < c.c_out) {
            const float bias = c.bias ? c.bias[co0 + q] : 0.f;
            yb[(long long)q * c.hw_out] = cg_act(s[q] + bias, c.act, c.slope);
        }
}

// What conv_gemm_f32 needs of a Conv2dGrad: blockIdx.z = rh * sw + rw.  Column (item, qh, qw) of the phase is input position
// (h0 + qh sh, w0 + qw sw); K index kk = (co * nth + tth) * ntw + ttw reads output position (uh - tth, uw - ttw) of channel co,
// (uh, uw) = ((h + ph) / sh, (w + pw) / sw).
struct Conv2dGradSrc {
    const Conv2dGrad& c;
    const int2* ktab;                               // [conv2d_grad_table_rows(kg)]: .x dy offset from (uh, uw), .y tth | ttw << 16
    const int rh = blockIdx.z / c.sw;
    const int rw = blockIdx.z - rh * c.sw;
    const int nth = phase_taps(c.kh, c.sh, rh), ntw = phase_taps(c.kw, c.sw, rw);
    const int kg = c.c_out * nth * ntw;
    const int h0 = phase_first(c.ph, c.sh, rh), w0 = phase_first(c.pw, c.sw, rw);
    const int nh = phase_count(c.h_in, c.sh, h0), nw = phase_count(c.w_in, c.sw, w0);
    const long long per_item = (long long)nh * nw;
    const long long ncols = (long long)c.n_items * per_item;
    long long ybase = 0;
    int uh = -0x40000000, uw = -0x40000000;         // an invalid column fails every bounds test
    __device__ int k_extent() const { return kg; }
    __device__ int m_extent() const { return c.c_in; }
    __device__ long long n_cols() const { return ncols; }
    __device__ const float* weights() const {
        const size_t taps = (size_t)phase_taps_before(c.kh, c.sh, rh) * c.kw + (size_t)nth * phase_taps_before(c.kw, c.sw, rw);
        return c.w + taps * c.c_out * c.c_in;                   // the phases before (rh, rw), rh major
    }
    __device__ void column(long long col) {
        if (col < ncols) {
            const long long item = col / per_item, rem = col - item * per_item;
            const int qh = (int)(rem / nw), qw = (int)(rem - (long long)qh * nw);
            uh = (h0 + qh * c.sh + c.ph) / c.sh;
            uw = (w0 + qw * c.sw + c.pw) / c.sw;
            ybase = item * c.c_out * c.hw_out + (long long)uh * c.w_out + uw;
        }
    }
    __device__ float tap(int kk) const {
        const int2 e = ktab[kk];
        const int ho = uh - (e.y & 0xffff), wo = uw - (e.y >> 16);
        const bool ok = e.y >= 0 && (unsigned)ho < (unsigned)c.h_out && (unsigned)wo < (unsigned)c.w_out;
        return ok ? cg_dz(c.dy, c.y, c.act, c.slope, ybase + e.x) : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / per_item, rem = n - item * per_item;
        const long long qh = rem / nw, qw = rem - qh * nw;
        return c.dx + item * c.c_in * c.hw_in + ((long long)h0 + qh * c.sh) * c.w_in + w0 + qw * c.sw;
    }
    __device__ long long out_stride() const { return c.hw_in; }
    __device__ int bias_index(int m) const { return m; }
};

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void conv2d_gemm_grad_kernel(Conv2dGrad c) {
    extern __shared__ int2 ktab[];
    Conv2dGradSrc src{c, ktab};
    if ((long long)blockIdx.x * (WN * TN * 32) >= src.ncols) return;            // the grid is sized for the phase with most columns
    const int per_co = src.nth * src.ntw;
    for (int kk = threadIdx.x; kk < conv2d_grad_table_rows(src.kg); kk += CG_THREADS) {
        int2 e = make_int2(0, -1);                             // past K: never loaded
        if (kk < src.kg) {
            const int co = kk / per_co, r = kk - co * per_co;
            const int tth = r / src.ntw, ttw = r - tth * src.ntw;
            e = make_int2((co * c.h_out - tth) * c.w_out - ttw, tth | (ttw << 16));
        }
        ktab[kk] = e;
    }
    __syncthreads();
    conv_gemm_f32<WM, WN, TM, TN>(src, nullptr, CG_ACT_NONE, 0.f);
}

// One dx element per thread; w is the reference's layout [c_out][c_in][kh][kw].
__global__ __launch_bounds__(CG_THREADS) void conv2d_direct_grad_kernel(Conv2dGrad c) {
    const long long o = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
    const long long total = (long long)c.n_items * c.c_in * c.hw_in;
    if (o >= total) return;
    const long long rem = o % c.hw_in, t = o / c.hw_in;
    const int ci = (int)(t % c.c_in);
    const long long item = t / c.c_in;
    const int h = (int)(rem / c.w_in), w = (int)(rem - (long long)h * c.w_in);
    const int rh = (h + c.ph) % c.sh, uh = (h + c.ph) / c.sh;
    const int rw = (w + c.pw) % c.sw, uw = (w + c.pw) / c.sw;
    const int khw = c.kh * c.kw;
    float s = 0.f;
    for (int co = 0; co < c.c_out; ++co) {
        const float* __restrict__ wr = c.w + ((size_t)co * c.c_in + ci) * khw;
        const long long base = (item * c.c_out + co) * c.hw_out;
        int ho = uh;
        for (int th = rh; th < c.kh && ho >= 0; th += c.sh, --ho) {
            if (ho >= c.h_out) continue;
            int wo = uw;
            for (int tw = rw; tw < c.kw && wo >= 0; tw += c.sw, --wo)
                if (wo < c.w_out)
                    s = fmaf(wr[th * c.kw + tw], cg_dz(c.dy, c.y, c.act, c.slope, base + (long long)ho * c.w_out + wo), s);
        }
    }
    c.dx[o] = s;
}

template <int WM, int WN, int TM, int TN>
static void launch_conv2d_gemm(const Conv2dArgs& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((c.n_cols + BN - 1) / BN), (unsigned)((c.c_out + BM - 1) / BM), 1);
    hipLaunchKernelGGL((conv2d_gemm_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), (size_t)conv2d_table_rows(c.kg) * sizeof(int2), s, c);
}

template <int WM, int WN, int TM, int TN>
static void launch_conv2d_gemm_grad(const Conv2dGrad& c, long long max_cols, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((max_cols + BN - 1) / BN), (unsigned)((c.c_in + BM - 1) / BM), (unsigned)(c.sh * c.sw));
    const int max_kg = c.c_out * phase_taps(c.kh, c.sh, 0) * phase_taps(c.kw, c.sw, 0);          // phase (0, 0) has the most taps
    hipLaunchKernelGGL((conv2d_gemm_grad_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS),
                       (size_t)conv2d_grad_table_rows(max_kg) * sizeof(int2), s, c);
}

// The checks adk_conv2d and adk_conv2d_grad both make of a layer, in their order, and its geometry.  `masked`: the backward,
// which takes the LeakyReLU mask from the layer's output and so needs slope >= 0.  The direction's own size limits and its
// pointers are the caller's to check next.
static int conv2d_geometry(const std::string& f, int n_items, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int sh, int sw,
                           int ph, int pw, int act, float slope, int impl, bool masked, Conv2dGeom& g) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || w_in <= 0 || c_out <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return fail(ADK_ERR_ARG, f + ": need n_items >= 0, c_in, h_in, w_in, c_out, kh, kw, sh, sw > 0, ph, pw >= 0");
    const int rc = cg_check_act_impl(f, act, slope, impl, masked);
    if (rc != ADK_OK) return rc;
    if (kh >= 32768 || kw >= 32768) return fail(ADK_ERR_ARG, f + ": kernel too large");
    const long long span_h = (long long)h_in + 2LL * ph - kh, span_w = (long long)w_in + 2LL * pw - kw;
    if (span_h < 0 || span_w < 0) return fail(ADK_ERR_SHAPE, f + ": kernel larger than the padded input");
    const long long h_out = span_h / sh + 1, w_out = span_w / sw + 1;
    g.n_items = n_items; g.c_in = c_in; g.h_in = h_in; g.w_in = w_in; g.c_out = c_out;
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw;
    g.h_out = (int)h_out; g.w_out = (int)w_out; g.act = act; g.slope = slope;
    g.hw_in = (long long)h_in * w_in; g.hw_out = h_out * w_out;
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_spectrogram_frames(int32_t n_samples, int32_t pad, int32_t hop) {
    if (n_samples <= 0 || pad < 0 || hop <= 0) return fail(ADK_ERR_ARG, "adk_spectrogram_frames: need n_samples > 0, pad >= 0, hop > 0");
    return spec_frames(n_samples, pad, hop);
}

extern "C" int adk_spectrogram(const float* x, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop,
                               const float* window, int32_t win_length, float* out, void* stream) {
    const std::string f = "adk_spectrogram";
    int rc = check_spec_args(f, n_signals, n_samples, pad, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "x/window/out", n_signals > 0 && (!x || !out), {x, window, out});
    if (rc != ADK_OK) return rc;
    if (n_signals == 0) return ADK_OK;
    const SpecArgs a(n_samples, pad, n_fft, hop, window, win_length);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(out));
    dispatch_log2n(n_fft, [&](auto L) {
        hipLaunchKernelGGL(spec_kernel<decltype(L)::value>, dim3(spec_workgroups(a, n_signals)), dim3(FFT_WAVE), 0, s, x, n_signals, a, out);
    });
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int64_t adk_spectrogram_grad_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || pad < 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_spectrogram_grad_workspace_bytes: need n_signals >= 0, n_samples > 0, pad >= 0, hop > 0, n_fft > 0");
    return (int64_t)n_signals * spec_frames(n_samples, pad, hop) * n_fft * (int64_t)sizeof(float);
}

extern "C" int adk_spectrogram_grad(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft,
                                    int32_t hop, const float* window, int32_t win_length, void* workspace, float* grad_x,
                                    void* stream) {
    const std::string f = "adk_spectrogram_grad";
    int rc = check_spec_args(f, n_signals, n_samples, pad, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    rc = check_pointers(f, "x/g/window/workspace/grad_x", n_signals > 0 && (!x || !g || !workspace || !grad_x),
                           {x, g, window, workspace, grad_x});
    if (rc != ADK_OK) return rc;
    if (n_signals == 0) return ADK_OK;
    const SpecArgs a(n_samples, pad, n_fft, hop, window, win_length);
    float* slab = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad_x));
    dispatch_log2n(n_fft, [&](auto L) {
        hipLaunchKernelGGL(spec_grad_frames_kernel<decltype(L)::value>, dim3(spec_workgroups(a, n_signals)), dim3(FFT_WAVE), 0, s, x, g,
                           n_signals, a, slab);
    });
    ADK_HIP_CHECK(hipGetLastError());
    launch_frame_grad_gather(slab, n_signals, n_samples, pad, n_fft, hop, a.frames, grad_x, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_conv2d(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t h_in,
                          int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                          int32_t act, float slope, int32_t impl, void* stream) {
    const std::string f = "adk_conv2d";
    Conv2dArgs c;
    int rc = conv2d_geometry(f, n_items, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, act, slope, impl, false, c);
    if (rc != ADK_OK) return rc;
    const long long kg = (long long)c_in * kh * kw;
    if ((long long)c_in * c.hw_in >= (1LL << 31) || (long long)c_out * c.hw_out >= (1LL << 40) || kg >= (1LL << 30) ||
        (long long)h_in * sh >= (1LL << 30) || (long long)w_in * sw >= (1LL << 30))
        return fail(ADK_ERR_ARG, f + ": layer too large");
    rc = check_pointers(f, "x/w/bias/y", n_items > 0 && (!x || !w || !y), {x, w, bias, y});
    if (rc != ADK_OK) return rc;
    c.x = x; c.w = w; c.bias = bias; c.y = y;
    c.kg = (int)kg;
    c.n_cols = (long long)n_items * c.hw_out;
    if (impl == CG_IMPL_DIRECT) {
        if ((c.n_cols + CG_THREADS - 1) / CG_THREADS >= (1LL << 31) || (c_out + 7) / 8 > 65535)
            return fail(ADK_ERR_ARG, f + ": layer too large for the direct kernel");
    } else {
        if (kg > UD_MAX_K) return fail(ADK_ERR_ARG, f + ": c_in * kh * kw > 4096 is beyond the gemm kernel's tap table");
        if ((c.n_cols + 127) / 128 >= (1LL << 31) || (c_out + 31) / 32 > 65535)
            return fail(ADK_ERR_ARG, f + ": layer too large for the gemm kernel");
    }
    if (n_items == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(y));
    if (impl == CG_IMPL_DIRECT) {
        const unsigned nb = (unsigned)((c.n_cols + CG_THREADS - 1) / CG_THREADS);
        if (c_out >= 8) hipLaunchKernelGGL(conv2d_direct_kernel<8>, dim3(nb, (unsigned)((c_out + 7) / 8)), dim3(CG_THREADS), 0, s, c);
        else hipLaunchKernelGGL(conv2d_direct_kernel<1>, dim3(nb, (unsigned)c_out), dim3(CG_THREADS), 0, s, c);
    } else {
        launch_conv2d_gemm<1, 4, 1, 1>(c, s);                          // 32 x 128; wider c_out takes more grid rows
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_conv2d_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t h_in,
                               int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                               int32_t act, float slope, int32_t impl, void* stream) {
    const std::string f = "adk_conv2d_grad";
    Conv2dGrad c;
    int rc = conv2d_geometry(f, n_items, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, act, slope, impl, true, c);
    if (rc != ADK_OK) return rc;
    const long long kg = (long long)c_out * kh * kw;
    if ((long long)c_in * c.hw_in >= (1LL << 31) || (long long)c_out * c.hw_out >= (1LL << 31) || kg >= (1LL << 30) ||
        (long long)h_in + ph + sh >= (1LL << 30) || (long long)w_in + pw + sw >= (1LL << 30) || (long long)sh * sw >= (1LL << 30))
        return fail(ADK_ERR_ARG, f + ": layer too large");
    rc = check_pointers(f, "dy/y/w/dx", n_items > 0 && (!dy || !w || !dx || (act == CG_ACT_LEAKY && !y)), {dy, y, w, dx});
    if (rc != ADK_OK) return rc;
    c.dy = dy; c.y = y; c.w = w; c.dx = dx;
    const long long total = (long long)n_items * c_in * c.hw_in;
    const long long max_cols = (long long)n_items * ((h_in + sh - 1) / sh) * ((w_in + sw - 1) / sw);   // the phase with h0 = w0 = 0
    if (impl == CG_IMPL_DIRECT) {
        if ((total + CG_THREADS - 1) / CG_THREADS >= (1LL << 31))
            return fail(ADK_ERR_ARG, f + ": layer too large for the direct kernel");
    } else {
        if (kg > UD_MAX_K) return fail(ADK_ERR_ARG, f + ": c_out * kh * kw > 4096 is beyond the gemm kernel's tap table");
        if ((max_cols + 127) / 128 >= (1LL << 31) || (c_in + 31) / 32 > 65535 || (long long)sh * sw > 65535)
            return fail(ADK_ERR_ARG, f + ": layer too large for the gemm kernel");
    }
    if (n_items == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(dx));
    if (impl == CG_IMPL_DIRECT)
        hipLaunchKernelGGL(conv2d_direct_grad_kernel, dim3((unsigned)((total + CG_THREADS - 1) / CG_THREADS)), dim3(CG_THREADS), 0, s, c);
    else
        launch_conv2d_gemm_grad<1, 4, 1, 1>(c, max_cols, s);             // 32 x 128; wider c_in takes more grid rows
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
