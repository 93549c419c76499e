// UnivNet spectral discriminator backward to its input (the gradient of the generator-side GAN losses with respect to y_hat
// through univ_disc.hip's 2-D convs and magnitude spectrogram; the weights are constants), exact f32, in gather form: every
// output element is written exactly once by one thread or one accumulator, nothing is added atomically, so the gradient is
// bitwise reproducible.  The period half's backward is disc_grad.hip's.
//
//   dx[i][ci][h][w] = sum over co and taps (th, tw) with (h + ph - th) % sh == 0, (w + pw - tw) % sw == 0,
//                     0 <= ho = (h + ph - th) / sh < H', 0 <= wo = (w + pw - tw) / sw < W'
//                     of W[co][ci][th][tw] dz[i][co][ho][wo],   dz = dy * (act ? (y > 0 ? 1 : slope) : 1)
//   (y the layer's saved post-activation output: y > 0 exactly where its pre-activation is, for slope >= 0).
//
//   conv2d_gemm_grad_kernel:   that sum as a GEMM through conv_gemm_f32.h's core:  M = C_in (rows of dx), N = input positions,
//                              K = (co, tap) pairs, split by PHASE (rh, rw) = ((h + ph) % sh, (w + pw) % sw) as disc_grad.hip
//                              splits its one axis: only the taps th = rh + tth sh, tw = rw + ttw sw reach such a position, so
//                              the columns are enumerated per phase, blockIdx.z = rh * sw + rw runs over the phases and the K
//                              loop of a grid slice runs over c_out * taps(rh) * taps(rw) pairs only -- no structural zero is
//                              multiplied.  W is re-packed once per layer to [phase][kk = (co * taps(rh) + tth) * taps(rw) + ttw][m];
//                              kk -> (dy offset, tth, ttw) comes from a table in dynamic LDS built per workgroup for its phase
//                              (no division in the K loop).  A phase without taps (kernel < stride on an axis) has K = 0 and
//                              writes zeros; so do rows and columns the forward never read (every ho or wo out of range).  The
//                              activation mask is applied where a tap is staged (Conv2dGradSrc::tap).
//   conv2d_direct_grad_kernel: one thread per dx element, for the C_in = 1 first layer -- whose dx is the spectrogram's gradient
//                              -- and the C_out = 1 output layer; written for any layer shape.
//   spec_grad_frames_kernel:   the vector-Jacobian product of spec_kernel, one frame per wave: the frame is recomputed exactly as
//                              spec_kernel loads it, bin k gets g[k] (re, im) / |X[k]| -- (0, 0) where |X[k]| == 0, torch's abs
//                              backward (sgn(0) = 0); a frame that lies in the zero padding has only such bins -- then
//                              stft_grad.h's tail into a slab [n_signals][frames][n_fft].
//   spec_grad_gather_kernel:   per sample, its contributions from the slab in ascending frame order.  Sample t is position
//                              p = t + pad of the zero-padded signal of length tp = T + 2 pad; the reflect padding acts on that
//                              longer signal, so p is also reached at -p and 2 (tp - 1) - p.
#include "conv_gemm_f32.h"
#include "stft_grad.h"

namespace adk {

constexpr int UDG_MAX_K = 4096;                     // GEMM: c_out * kh * kw, the rows of the largest phase's tap table bound
constexpr int UDG_SPEC_MAX_WG = 8192;

// ---- 2-D conv, backward-data ----
struct Conv2dGrad {
    const float* dy;                                // [n_items][c_out][h_out][w_out]
    const float* y;                                 // same shape: the forward's output (read when act is leaky)
    const float* w;
    float* dx;                                      // [n_items][c_in][h_in][w_in]
    int n_items, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, h_out, w_out, act;
    float slope;
    long long hw_in, hw_out;                        // positions per channel
};

// One axis of the phase split: taps r, r + s, ... < k of phase r; the taps of the phases before r; the first input index of
// phase r; how many of n input indices first, first + s, ... there are.
__host__ __device__ inline int phase_taps(int k, int s, int r) { return r < k ? (k - r + s - 1) / s : 0; }
__host__ __device__ inline int phase_taps_before(int k, int s, int r) { return (k / s) * r + (k % s < r ? k % s : r); }
__host__ __device__ inline int phase_first(int pad, int s, int r) { return ((r - pad) % s + s) % s; }
__host__ __device__ inline int phase_count(int n, int s, int first) { return first < n ? (n - first + s - 1) / s : 0; }

__device__ __forceinline__ float conv2d_dz(const Conv2dGrad& c, long long idx) {
    const float v = c.dy[idx];
    return (c.act == CG_ACT_LEAKY && !(c.y[idx] > 0.f)) ? v * c.slope : v;
}

// What conv_gemm_f32 needs of a Conv2dGrad: blockIdx.z = rh * sw + rw.  Column (item, qh, qw) of the phase is input position
// (h0 + qh sh, w0 + qw sw); K index kk = (co * nth + tth) * ntw + ttw reads output position (uh - tth, uw - ttw) of channel co,
// (uh, uw) = ((h + ph) / sh, (w + pw) / sw).
struct Conv2dGradSrc {
    const Conv2dGrad& c;
    const int2* ktab;                               // [kg rounded up to CG_KT, >= CG_KT]: .x dy offset from (uh, uw), .y tth | ttw << 16
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
        return ok ? conv2d_dz(c, ybase + e.x) : 0.f;
    }
    __device__ float* out(long long n) const {
        const long long item = n / per_item, rem = n - item * per_item;
        const long long qh = rem / nw, qw = rem - qh * nw;
        return c.dx + item * c.c_in * c.hw_in + ((long long)h0 + qh * c.sh) * c.w_in + w0 + qw * c.sw;
    }
    __device__ long long out_stride() const { return c.hw_in; }
    __device__ int bias_index(int m) const { return m; }
};

__host__ __device__ inline int udg_table_rows(int kg) { return kg > 0 ? (kg + CG_KT - 1) / CG_KT * CG_KT : CG_KT; }

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(CG_THREADS) void conv2d_gemm_grad_kernel(Conv2dGrad c) {
    extern __shared__ int2 ktab[];
    Conv2dGradSrc src{c, ktab};
    if ((long long)blockIdx.x * (WN * TN * 32) >= src.ncols) return;            // the grid is sized for the phase with most columns
    const int per_co = src.nth * src.ntw;
    for (int kk = threadIdx.x; kk < udg_table_rows(src.kg); kk += CG_THREADS) {
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
                if (wo < c.w_out) s = fmaf(wr[th * c.kw + tw], conv2d_dz(c, base + (long long)ho * c.w_out + wo), s);
        }
    }
    c.dx[o] = s;
}

template <int WM, int WN, int TM, int TN>
static void launch_conv2d_gemm_grad(const Conv2dGrad& c, long long max_cols, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((max_cols + BN - 1) / BN), (unsigned)((c.c_in + BM - 1) / BM), (unsigned)(c.sh * c.sw));
    const int max_kg = c.c_out * phase_taps(c.kh, c.sh, 0) * phase_taps(c.kw, c.sw, 0);          // phase (0, 0) has the most taps
    hipLaunchKernelGGL((conv2d_gemm_grad_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), (size_t)udg_table_rows(max_kg) * sizeof(int2),
                       s, c);
}

// ---- magnitude spectrogram, vector-Jacobian product ----
struct SpecGradArgs {
    int n_samples, pad, hop;
    long long frames;
};

template <int LOG2N>
__global__ __launch_bounds__(FFT_WAVE) void spec_grad_frames_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                    int n_signals, SpecGradArgs a, StftFrameArgs fa,
                                                                    float* __restrict__ slab) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N, HALF = NFFT / 2;
    __shared__ float2 tw[N + 2];
    __shared__ float buf[NFFT];
    __shared__ float2 keep[N + 2];
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long tp = (long long)a.n_samples + 2LL * a.pad;            // length of the zero-padded signal
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        const float* __restrict__ xs = x + (size_t)s * a.n_samples;
        const long long u0 = f * a.hop - HALF;
        // the frame as spec_kernel loads it
#pragma unroll 4
        for (int j = lane; j < NFFT; j += FFT_WAVE) {
            long long u = u0 + j;
            u = u < 0 ? -u : u;                                            // reflect padding of the zero-padded signal
            u = u >= tp ? 2LL * (tp - 1) - u : u;
            const long long t = u - a.pad;                                 // zero padding
            const int jw = j - fa.lpad;
            float v = 0.f;
            if (t >= 0 && t < a.n_samples && jw >= 0 && jw < fa.win_length) v = __fmul_rn(xs[t], fa.window[jw]);
            buf[j] = v;
        }
        __syncthreads();
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
        frame_grad_tail<LOG2N>(fa, buf, tw, keep, slab + (size_t)it * NFFT);
    }
}

// stft_grad.h's gather on the zero-padded signal: sample t is position p = t + pad of tp = T + 2 pad, reached at u = p and,
// through the reflect padding, at u = -p and u = 2 (tp - 1) - p where a frame reaches them; position u is float
// u - (f hop - n_fft/2) of frame f.  Frames in ascending order, positions in ascending order within a frame.
__global__ __launch_bounds__(GRAD_GATHER_THREADS) void spec_grad_gather_kernel(const float* __restrict__ slab, int n_signals, int T,
                                                                               int pad, int n_fft, int hop, long long frames,
                                                                               float* __restrict__ grad_x) {
    const long long total = (long long)n_signals * T, half = n_fft / 2, tp = (long long)T + 2LL * pad;
    for (long long e = (long long)blockIdx.x * GRAD_GATHER_THREADS + threadIdx.x; e < total;
         e += (long long)gridDim.x * GRAD_GATHER_THREADS) {
        const long long s = e / T, p = e - s * T + pad;
        const long long u[3] = {-p, p, 2LL * (tp - 1) - p};
        const bool on[3] = {p >= 1, true, p <= tp - 2};
        long long lo = frames, hi = -1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!on[i]) continue;
            const long long f0 = max(floor_div(u[i] - half, hop) + 1, 0LL), f1 = min(floor_div(u[i] + half, hop), frames - 1);
            if (f0 <= f1) { lo = min(lo, f0); hi = max(hi, f1); }
        }
        const float* fs = slab + (size_t)s * frames * n_fft;
        float acc = 0.f;
        for (long long f = lo; f <= hi; ++f) {
            const long long base = f * hop - half;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const long long j = u[i] - base;
                if (on[i] && j >= 0 && j < n_fft) acc += fs[(size_t)f * n_fft + j];
            }
        }
        grad_x[e] = acc;
    }
}

template <int LOG2N>
static void launch_spec_grad_frames(const float* x, const float* g, int n_signals, const SpecGradArgs& a, const StftFrameArgs& fa,
                                    float* slab, hipStream_t s) {
    const int n_wg = (int)std::min<long long>(a.frames * n_signals, UDG_SPEC_MAX_WG);
    hipLaunchKernelGGL(spec_grad_frames_kernel<LOG2N>, dim3(n_wg), dim3(FFT_WAVE), 0, s, x, g, n_signals, a, fa, slab);
}

// The checks adk_spectrogram makes of the arguments the backward shares with it.
static int check_spec_args(const std::string& f, int n_signals, int n_samples, int pad, int n_fft, int hop, int win_length) {
    const int rc = check_fft_sizes(f, n_fft, hop, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals < 0 || n_samples <= 0 || pad < 0) return fail(ADK_ERR_ARG, f + ": need n_signals >= 0, n_samples > 0, pad >= 0");
    if ((long long)n_samples + 2LL * pad <= n_fft / 2)
        return fail(ADK_ERR_ARG, f + ": reflect padding needs n_samples + 2 pad > n_fft / 2");
    if ((long long)n_samples + 2LL * pad >= (1LL << 31)) return fail(ADK_ERR_ARG, f + ": signal too long");
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int adk_conv2d_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t h_in,
                               int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                               int32_t act, float slope, int32_t impl, void* stream) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || w_in <= 0 || c_out <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return fail(ADK_ERR_ARG, "adk_conv2d_grad: need n_items >= 0, c_in, h_in, w_in, c_out, kh, kw, sh, sw > 0, ph, pw >= 0");
    if (act != CG_ACT_NONE && act != CG_ACT_LEAKY) return fail(ADK_ERR_ARG, "adk_conv2d_grad: act must be 0 (none) or 2 (leaky)");
    if (act == CG_ACT_LEAKY && !(slope >= 0.f))
        return fail(ADK_ERR_ARG, "adk_conv2d_grad: the mask is taken from the output, which needs slope >= 0");
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, "adk_conv2d_grad: impl must be 1 (direct) or 2 (gemm)");
    if (kh >= 32768 || kw >= 32768) return fail(ADK_ERR_ARG, "adk_conv2d_grad: kernel too large");
    const long long span_h = (long long)h_in + 2LL * ph - kh, span_w = (long long)w_in + 2LL * pw - kw;
    if (span_h < 0 || span_w < 0) return fail(ADK_ERR_SHAPE, "adk_conv2d_grad: kernel larger than the padded input");
    const long long h_out = span_h / sh + 1, w_out = span_w / sw + 1;
    const long long kg = (long long)c_out * kh * kw;
    if ((long long)c_in * h_in * w_in >= (1LL << 31) || (long long)c_out * h_out * w_out >= (1LL << 31) || kg >= (1LL << 30) ||
        (long long)h_in + ph + sh >= (1LL << 30) || (long long)w_in + pw + sw >= (1LL << 30) || (long long)sh * sw >= (1LL << 30))
        return fail(ADK_ERR_ARG, "adk_conv2d_grad: layer too large");
    if (n_items > 0 && (!dy || !w || !dx || (act == CG_ACT_LEAKY && !y))) return fail(ADK_ERR_ARG, "adk_conv2d_grad: null pointer");
    if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w) |
         reinterpret_cast<uintptr_t>(dx)) & 3)
        return fail(ADK_ERR_ARG, "adk_conv2d_grad: dy/y/w/dx must be 4-byte aligned");
    Conv2dGrad c;
    c.dy = dy; c.y = y; c.w = w; c.dx = dx;
    c.n_items = n_items; c.c_in = c_in; c.h_in = h_in; c.w_in = w_in; c.c_out = c_out;
    c.kh = kh; c.kw = kw; c.sh = sh; c.sw = sw; c.ph = ph; c.pw = pw;
    c.h_out = (int)h_out; c.w_out = (int)w_out; c.act = act; c.slope = slope;
    c.hw_in = (long long)h_in * w_in; c.hw_out = h_out * w_out;
    const long long total = (long long)n_items * c_in * c.hw_in;
    const long long max_cols = (long long)n_items * ((h_in + sh - 1) / sh) * ((w_in + sw - 1) / sw);   // the phase with h0 = w0 = 0
    if (impl == CG_IMPL_DIRECT) {
        if ((total + CG_THREADS - 1) / CG_THREADS >= (1LL << 31))
            return fail(ADK_ERR_ARG, "adk_conv2d_grad: layer too large for the direct kernel");
    } else {
        if (kg > UDG_MAX_K) return fail(ADK_ERR_ARG, "adk_conv2d_grad: c_out * kh * kw > 4096 is beyond the gemm kernel's tap table");
        if ((max_cols + 127) / 128 >= (1LL << 31) || (c_in + 31) / 32 > 65535 || (long long)sh * sw > 65535)
            return fail(ADK_ERR_ARG, "adk_conv2d_grad: layer too large for the gemm kernel");
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

extern "C" int64_t adk_spectrogram_grad_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || pad < 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_spectrogram_grad_workspace_bytes: need n_signals >= 0, n_samples > 0, pad >= 0, hop > 0, n_fft > 0");
    return (int64_t)n_signals * (1 + ((int64_t)n_samples + 2LL * pad) / hop) * n_fft * (int64_t)sizeof(float);
}

extern "C" int adk_spectrogram_grad(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft,
                                    int32_t hop, const float* window, int32_t win_length, void* workspace, float* grad_x,
                                    void* stream) {
    const int rc = check_spec_args("adk_spectrogram_grad", n_signals, n_samples, pad, n_fft, hop, win_length);
    if (rc != ADK_OK) return rc;
    if (!window) return fail(ADK_ERR_ARG, "adk_spectrogram_grad: null window");
    if (n_signals > 0 && (!x || !g || !workspace || !grad_x)) return fail(ADK_ERR_ARG, "adk_spectrogram_grad: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(window) |
         reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(grad_x)) & 3)
        return fail(ADK_ERR_ARG, "adk_spectrogram_grad: x/g/window/workspace/grad_x must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    SpecGradArgs a;
    a.n_samples = n_samples; a.pad = pad; a.hop = hop;
    a.frames = 1 + ((long long)n_samples + 2LL * pad) / hop;
    const StftFrameArgs fa(n_samples, n_fft, hop, window, win_length, 0.f);       // the window's placement, for the shared tail
    float* slab = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad_x));
    dispatch_log2n(n_fft, [&](auto L) { launch_spec_grad_frames<decltype(L)::value>(x, g, n_signals, a, fa, slab, s); });
    ADK_HIP_CHECK(hipGetLastError());
    const long long total = (long long)n_signals * n_samples;
    const int n_wg = (int)std::min<long long>((total + GRAD_GATHER_THREADS - 1) / GRAD_GATHER_THREADS, GRAD_GATHER_MAX_WG);
    hipLaunchKernelGGL(spec_grad_gather_kernel, dim3(n_wg), dim3(GRAD_GATHER_THREADS), 0, s, slab, n_signals, n_samples, pad, n_fft, hop,
                       a.frames, grad_x);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
