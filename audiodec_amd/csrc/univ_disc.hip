// UnivNet spectral discriminator forward (models/vocoder/modules/discriminator.py:451-640), exact f32: the magnitude
// spectrogram front end and the true 2-D convs over (frames, bins) planes.  The period half of the UnivNet discriminator and
// the loss sums are disc.hip's.
//
//   spec_kernel:         torchaudio.functional.spectrogram(x, pad, window, n_fft, hop, win_length, power=1) transposed:
//                        frame f of signal s = xp[f*hop - n_fft/2 + j] (reflected at both ends of xp) * window_centred[j], where
//                        xp is x with `pad` zeros on both sides (never materialised: both paddings and the window are applied
//                        while loading); out [s][f][k] = |X_f[k]|, k <= n_fft/2, no eps clamp.  One frame per wave, the FFT of
//                        fft_wave.h; a frame's bins are one coalesced run of the output.  The load loop is this kernel's own and not
//                        stft_frame.h's: it zero-pads inside the reflect padding and writes a literal 0 outside the window.
//   conv2d_gemm_kernel:  x [n][c_in][H][W] -> y [n][c_out][H'][W'], kernel (kh, kw), stride (sh, sw), zero padding (ph, pw) by
//                        predicated loads, as an implicit GEMM through conv_gemm_f32.h's core:
//                          Y[m][n] = bias[m] + sum_kk W[kk][m] X[kk][n],  m < c_out,  kk = (ci*kh + th)*kw + tw,
//                          n = (item, h', w');  X[kk][n] = x[item][ci][h'*sh - ph + th][w'*sw - pw + tw]
//                        Conv2dSrc is that addressing; the wrapper builds its kk table once per workgroup in LDS.
//   conv2d_direct_kernel: one thread per output position and block of COB output channels, for the c_in = 1 first layer and
//                        the c_out = 1 output layer, where a GEMM tile would be mostly padding.  Same k order.
#include "conv_gemm_f32.h"
#include "stft_frame.h"

namespace adk {

constexpr int UD_MAX_K = 4096;                      // GEMM: rows of the kk table (8 bytes each in LDS)
constexpr int UD_SPEC_MAX_WG = 8192;

// ---- magnitude spectrogram ----
struct SpecArgs {
    int n_samples, pad, hop, win_length, lpad;
    long long frames;
    const float* window;
};

template <int LOG2N>
__global__ __launch_bounds__(FFT_WAVE) void spec_kernel(const float* __restrict__ x, int n_signals, SpecArgs a,
                                                        float* __restrict__ out) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N, HALF = NFFT / 2;
    __shared__ float2 tw[N + 2];
    __shared__ float buf[NFFT];
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long tp = (long long)a.n_samples + 2LL * a.pad;            // length of the zero-padded signal
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        const float* __restrict__ xs = x + (size_t)s * a.n_samples;
        const long long u0 = f * a.hop - HALF;
#pragma unroll 4
        for (int j = lane; j < NFFT; j += FFT_WAVE) {
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
static void launch_spec(const float* x, int n_signals, const SpecArgs& a, float* out, hipStream_t s) {
    const int n_wg = (int)std::min<long long>(a.frames * n_signals, UD_SPEC_MAX_WG);
    hipLaunchKernelGGL(spec_kernel<LOG2N>, dim3(n_wg), dim3(FFT_WAVE), 0, s, x, n_signals, a, out);
}

// ---- 2-D conv ----
struct Conv2dArgs {
    const float* x;
    const float* w;
    const float* bias;                              // [c_out] or null
    float* y;
    int n_items, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, h_out, w_out, act;
    int kg;                                         // c_in * kh * kw: GEMM K
    float slope;
    long long hw_in, hw_out;                        // positions per channel
    long long n_cols;                               // n_items * hw_out: GEMM N
};

// What conv_gemm_f32 needs of a Conv2dArgs: both axes have taps and strides, so kk -> (input offset, th, tw) comes from ktab,
// a table in dynamic LDS (no division in the K loop), and a column gives (item base, h0, w0).
struct Conv2dSrc {
    const Conv2dArgs& c;
    const int2* ktab;                               // [kg rounded up to CG_KT]: .x input offset of tap kk, .y th | tw << 16
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
    const int n_kt = (c.kg + CG_KT - 1) / CG_KT;
    const int khw = c.kh * c.kw;
    for (int kk = threadIdx.x; kk < n_kt * CG_KT; kk += CG_THREADS) {
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

template <int WM, int WN, int TM, int TN>
static void launch_conv2d_gemm(const Conv2dArgs& c, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((c.n_cols + BN - 1) / BN), (unsigned)((c.c_out + BM - 1) / BM), 1);
    const size_t tab = (size_t)((c.kg + CG_KT - 1) / CG_KT) * CG_KT * sizeof(int2);
    hipLaunchKernelGGL((conv2d_gemm_kernel<WM, WN, TM, TN>), grid, dim3(CG_THREADS), tab, s, c);
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_spectrogram_frames(int32_t n_samples, int32_t pad, int32_t hop) {
    if (n_samples <= 0 || pad < 0 || hop <= 0) return fail(ADK_ERR_ARG, "adk_spectrogram_frames: need n_samples > 0, pad >= 0, hop > 0");
    return 1 + ((int64_t)n_samples + 2LL * pad) / hop;
}

extern "C" int adk_spectrogram(const float* x, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop,
                               const float* window, int32_t win_length, float* out, void* stream) {
    const int rc = check_fft_sizes("adk_spectrogram", n_fft, hop, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals < 0 || n_samples <= 0 || pad < 0) return fail(ADK_ERR_ARG, "adk_spectrogram: need n_signals >= 0, n_samples > 0, pad >= 0");
    if ((long long)n_samples + 2LL * pad <= n_fft / 2)
        return fail(ADK_ERR_ARG, "adk_spectrogram: reflect padding needs n_samples + 2 pad > n_fft / 2");
    if ((long long)n_samples + 2LL * pad >= (1LL << 31)) return fail(ADK_ERR_ARG, "adk_spectrogram: signal too long");
    if (!window) return fail(ADK_ERR_ARG, "adk_spectrogram: null window");
    if (n_signals > 0 && (!x || !out)) return fail(ADK_ERR_ARG, "adk_spectrogram: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(window) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(ADK_ERR_ARG, "adk_spectrogram: x/window/out must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    SpecArgs a;
    a.n_samples = n_samples; a.pad = pad; a.hop = hop; a.win_length = win_length; a.lpad = (n_fft - win_length) / 2;
    a.frames = 1 + ((long long)n_samples + 2LL * pad) / hop;
    a.window = window;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(out));
    dispatch_log2n(n_fft, [&](auto L) { launch_spec<decltype(L)::value>(x, n_signals, a, out, s); });
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_conv2d(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t h_in,
                          int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                          int32_t act, float slope, int32_t impl, void* stream) {
    if (n_items < 0 || c_in <= 0 || h_in <= 0 || w_in <= 0 || c_out <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0)
        return fail(ADK_ERR_ARG, "adk_conv2d: need n_items >= 0, c_in, h_in, w_in, c_out, kh, kw, sh, sw > 0, ph, pw >= 0");
    if (act != CG_ACT_NONE && act != CG_ACT_LEAKY) return fail(ADK_ERR_ARG, "adk_conv2d: act must be 0 (none) or 2 (leaky)");
    if (impl != CG_IMPL_DIRECT && impl != CG_IMPL_GEMM) return fail(ADK_ERR_ARG, "adk_conv2d: impl must be 1 (direct) or 2 (gemm)");
    if (kh >= 32768 || kw >= 32768) return fail(ADK_ERR_ARG, "adk_conv2d: kernel too large");
    const long long span_h = (long long)h_in + 2LL * ph - kh, span_w = (long long)w_in + 2LL * pw - kw;
    if (span_h < 0 || span_w < 0) return fail(ADK_ERR_SHAPE, "adk_conv2d: kernel larger than the padded input");
    const long long h_out = span_h / sh + 1, w_out = span_w / sw + 1;
    const long long kg = (long long)c_in * kh * kw;
    if ((long long)c_in * h_in * w_in >= (1LL << 31) || (long long)c_out * h_out * w_out >= (1LL << 40) || kg >= (1LL << 30) ||
        (long long)h_in * sh >= (1LL << 30) || (long long)w_in * sw >= (1LL << 30))
        return fail(ADK_ERR_ARG, "adk_conv2d: layer too large");
    if (n_items > 0 && (!x || !w || !y)) return fail(ADK_ERR_ARG, "adk_conv2d: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) |
         reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_conv2d: x/w/bias/y must be 4-byte aligned");
    Conv2dArgs c;
    c.x = x; c.w = w; c.bias = bias; c.y = y;
    c.n_items = n_items; c.c_in = c_in; c.h_in = h_in; c.w_in = w_in; c.c_out = c_out;
    c.kh = kh; c.kw = kw; c.sh = sh; c.sw = sw; c.ph = ph; c.pw = pw;
    c.h_out = (int)h_out; c.w_out = (int)w_out; c.act = act; c.slope = slope; c.kg = (int)kg;
    c.hw_in = (long long)h_in * w_in; c.hw_out = h_out * w_out;
    c.n_cols = (long long)n_items * c.hw_out;
    if (impl == CG_IMPL_DIRECT) {
        if ((c.n_cols + CG_THREADS - 1) / CG_THREADS >= (1LL << 31) || (c_out + 7) / 8 > 65535)
            return fail(ADK_ERR_ARG, "adk_conv2d: layer too large for the direct kernel");
    } else {
        if (kg > UD_MAX_K) return fail(ADK_ERR_ARG, "adk_conv2d: c_in * kh * kw > 4096 is beyond the gemm kernel's tap table");
        if ((c.n_cols + 127) / 128 >= (1LL << 31) || (c_out + 31) / 32 > 65535)
            return fail(ADK_ERR_ARG, "adk_conv2d: layer too large for the gemm kernel");
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
