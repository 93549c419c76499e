// How a torch.stft frame is made (center=True, reflect padding of n_fft/2, one-sided, no normalisation, the window zero-padded to
// n_fft and centred), for the one-wave frame kernels of mel.hip and stft_loss.hip:
//   frame f of signal x = x[f*hop - n_fft/2 + j] (reflected at both ends) * window_centred[j],   j < n_fft,  1 + T/hop frames
//   amp[k] = sqrt(clamp(re^2 + im^2, eps)),  k <= n_fft/2
// The frame lives in LDS and never leaves its wave; the FFT is fft_wave.h's.  Host side: the argument checks every frame entry
// point shares and the one dispatch from n_fft to the kernels' LOG2N.
#pragma once
#include <type_traits>
#include "adk_common.h"
#include "fft_wave.h"

namespace adk {

static inline long long stft_frames(int n_samples, int hop) { return 1 + (long long)n_samples / hop; }

struct StftFrameArgs {
    int n_samples, hop, win_length, lpad;
    long long frames;
    float eps;
    const float* window;
    StftFrameArgs(int n_samples_, int n_fft, int hop_, const float* window_, int win_length_, float eps_)
        : n_samples(n_samples_), hop(hop_), win_length(win_length_), lpad((n_fft - win_length_) / 2),
          frames(stft_frames(n_samples_, hop_)), eps(eps_), window(window_) {}
};

// A frame kernel's dynamic LDS: N + 1 twiddles (padded to N + 2), the frame's n_fft floats, then whatever the kernel adds.
template <int LOG2N>
struct FrameLds {
    static constexpr int N = 1 << LOG2N, NFFT = 2 << LOG2N;
    static __device__ __forceinline__ float2* tw(float* lds) { return reinterpret_cast<float2*>(lds); }
    static __device__ __forceinline__ float* buf(float* lds) { return lds + 2 * (N + 2); }
    static __device__ __forceinline__ float* extra(float* lds) { return lds + 2 * (N + 2) + NFFT; }
    static size_t bytes(size_t extra_floats = 0) { return sizeof(float) * (2 * (N + 2) + NFFT + extra_floats); }
};

// Bins per lane: lane l holds bins k = l + 64 q <= N.
template <int LOG2N>
constexpr int FRAME_PER = ((1 << LOG2N) + FFT_WAVE) / FFT_WAVE;

// clamp(v, min=eps) as torch.clamp: NaN stays NaN
__device__ __forceinline__ float clamp_min(float v, float eps) { return v < eps ? eps : v; }

// Frame f of signal x into buf (n_fft floats of LDS) and its DIF spectrum in place (read it with frame_amplitudes).  Ends with a
// barrier.
template <int LOG2N>
__device__ __forceinline__ void frame_spectrum(const float* __restrict__ x, long long f, const StftFrameArgs& a, float* buf,
                                               const float2* tw) {
    constexpr int NFFT = 2 << LOG2N, HALF = NFFT / 2;
    const int lane = threadIdx.x;
    const long long t0 = f * a.hop - HALF;
    const int T = a.n_samples;
    // reflect padding and the centred zero-padded window at load time; sample j is float j of the complex buffer.  Outside the
    // window the product with 0 is kept, so a non-finite sample there gives NaN as it does in torch.
#pragma unroll 4
    for (int j = lane; j < NFFT; j += FFT_WAVE) {
        long long t = t0 + j;
        t = t < 0 ? -t : t;
        t = t >= T ? 2LL * (T - 1) - t : t;
        const int jw = j - a.lpad;
        const float w = (jw >= 0 && jw < a.win_length) ? a.window[jw] : 0.f;
        buf[j] = __fmul_rn(x[t], w);
    }
    __syncthreads();
    wave_fft_dif<LOG2N>(reinterpret_cast<float2*>(buf), tw);      // radix-2 DIF, ends with a barrier
}

// amp[q] = amplitude of bin k = lane + 64 q of the spectrum frame_spectrum left in buf (0 past the last bin), untangled through
// the bit reversal.  KEEP (the mel backward's recompute): also keep[k] = (re, im).  Ends with a barrier, so the caller may reuse
// buf at once.
template <int LOG2N, bool KEEP = false>
__device__ __forceinline__ void frame_amplitudes(const float* buf, const float2* tw, float eps, float (&amp)[FRAME_PER<LOG2N>],
                                                 float2* keep = nullptr) {
    constexpr int N = 1 << LOG2N;
    const int lane = threadIdx.x;
    const float2* z = reinterpret_cast<const float2*>(buf);
#pragma unroll
    for (int q = 0; q < FRAME_PER<LOG2N>; ++q) {
        const int k = lane + q * FFT_WAVE;
        amp[q] = 0.f;
        if (k <= N) {
            float re, im;
            wave_fft_bin<LOG2N>(z, tw, k, re, im);
            amp[q] = sqrtf(clamp_min(re * re + im * im, eps));
            if constexpr (KEEP) keep[k] = make_float2(re, im);
        }
    }
    __syncthreads();
}

// ---- host side ----

// f(std::integral_constant<int, LOG2N>) for a checked n_fft = 2 << LOG2N in [256, 4096].
template <class F>
static inline void dispatch_log2n(int n_fft, F&& f) {
    switch (n_fft) {
        case 256: f(std::integral_constant<int, 7>{}); break;
        case 512: f(std::integral_constant<int, 8>{}); break;
        case 1024: f(std::integral_constant<int, 9>{}); break;
        case 2048: f(std::integral_constant<int, 10>{}); break;
        default: f(std::integral_constant<int, 11>{}); break;
    }
}

static inline int check_fft_sizes(const std::string& f, int n_fft, int hop, int win_length) {
    if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return fail(ADK_ERR_ARG, f + ": n_fft must be a power of two in [256, 4096]");
    if (hop <= 0) return fail(ADK_ERR_ARG, f + ": need hop > 0");
    if (win_length <= 0 || win_length > n_fft) return fail(ADK_ERR_ARG, f + ": need 0 < win_length <= n_fft");
    return ADK_OK;
}

static inline int check_stft_args(const char* fn, int n_signals, int n_samples, int n_fft, int hop, const float* window,
                                  int win_length) {
    const std::string f(fn);
    const int rc = check_fft_sizes(f, n_fft, hop, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals < 0) return fail(ADK_ERR_ARG, f + ": need n_signals >= 0");
    if (n_samples <= n_fft / 2) return fail(ADK_ERR_ARG, f + ": reflect padding needs n_samples > n_fft / 2");
    if (!window) return fail(ADK_ERR_ARG, f + ": null pointer");
    if (reinterpret_cast<uintptr_t>(window) & 3) return fail(ADK_ERR_ARG, f + ": window must be 4-byte aligned");
    return ADK_OK;
}

}  // namespace adk
