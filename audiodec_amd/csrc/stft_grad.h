// The tail every backward of a one-wave frame kernel ends in (mel.hip, stft_loss.hip, univ_disc.hip): from the per-bin gradients of a frame's
// spectrum to the gradient of the signal.
//   frame_grad_tail:  (g_re, g_im) of bins k <= n_fft/2 in keep[] -> transposed untangle -> transposed FFT (fft_wave.h) -> the
//                     centred window -> the frame's n_fft windowed gradients, one row of a slab [n_signals][frames][n_fft]
//   frame_grad_gather: a second launch that gathers, per sample, its contributions from the slab through the reflect padding in
//                     ascending frame order.  No float atomics, so the gradient is bitwise reproducible.
#pragma once
#include "stft_frame.h"

namespace adk {

// keep[k] = (d/d re, d/d im) of bin k <= N, written and synchronised by the caller; buf: the frame's n_fft floats of LDS
// (overwritten); out[j], j < n_fft, gets the windowed frame gradient.  Ends with a barrier.
template <int LOG2N>
__device__ __forceinline__ void frame_grad_tail(const StftFrameArgs& a, float* buf, const float2* tw, const float2* keep,
                                                float* __restrict__ out) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N;
    const int lane = threadIdx.x;
    // transposed untangle into the bit-reversed addresses, then the transposed FFT: natural order out, float j = sample j
    float2* z = reinterpret_cast<float2*>(buf);
    for (int p = lane; p < N; p += FFT_WAVE)
        z[__builtin_bitreverse32((unsigned)p) >> (32 - LOG2N)] = wave_fft_bin_t<LOG2N>(keep, tw, p);
    __syncthreads();
    wave_fft_dit_t<LOG2N>(z, tw);
#pragma unroll 4
    for (int j = lane; j < NFFT; j += FFT_WAVE) {
        const int jw = j - a.lpad;
        const float w = (jw >= 0 && jw < a.win_length) ? a.window[jw] : 0.f;
        out[j] = __fmul_rn(buf[j], w);
    }
    __syncthreads();
}

__device__ __forceinline__ long long floor_div(long long v, long long d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

// The overlap-add through the reflect padding, gathered.  The frames were cut from the signal with `pad` zeros on both sides
// (0 for torch.stft, univ_disc.hip's spectrogram pads), of length tp = T + 2 pad: sample t is its position p = t + pad, reached at
// u = p and, through the reflect padding of that longer signal, at u = -p (p >= 1) and u = 2 (tp - 1) - p (p <= tp - 2) where a
// frame reaches them; position u is float u - (f hop - n_fft/2) of frame f.  Frames in ascending order, positions in ascending
// order within a frame; a sample no frame reaches gets 0.
constexpr int GRAD_GATHER_THREADS = 256;
constexpr int GRAD_GATHER_MAX_WG = 32768;
static __global__ __launch_bounds__(GRAD_GATHER_THREADS) void frame_grad_gather_kernel(const float* __restrict__ slab,
                                                                                       int n_signals, int T, int pad, int n_fft,
                                                                                       int hop, long long frames,
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

// The gather launch over slab [n_signals][frames][n_fft] into grad [n_signals][n_samples].
static inline void launch_frame_grad_gather(const float* slab, int n_signals, int n_samples, int pad, int n_fft, int hop,
                                            long long frames, float* grad, hipStream_t s) {
    const long long total = (long long)n_signals * n_samples;
    const int n_wg = (int)std::min<long long>((total + GRAD_GATHER_THREADS - 1) / GRAD_GATHER_THREADS, GRAD_GATHER_MAX_WG);
    hipLaunchKernelGGL(frame_grad_gather_kernel, dim3(n_wg), dim3(GRAD_GATHER_THREADS), 0, s, slab, n_signals, n_samples, pad, n_fft,
                       hop, frames, grad);
}

}  // namespace adk
