// Multi-resolution STFT loss and waveform-shape loss (losses/stft_loss.py:19-170, losses/waveform_loss.py:15-75), one resolution
// or one window length per call.  The STFT is torch.stft's with its defaults (center=True, reflect padding of n_fft/2, one-sided,
// no normalisation, the window zero-padded to n_fft and centred):
//   frame f of signal s = x[s][f*hop - n_fft/2 + j] (reflected at both ends) * window_centred[j],   j < n_fft,  1 + T/hop frames
//   mag[k] = sqrt(clamp(re^2 + im^2, eps)),  k <= n_fft/2
// One frame is one wave64 workgroup; the frame load, the FFT and the clamped magnitudes are stft_frame.h's (shared with mel.hip),
// twiddles are built per workgroup in f64 and rounded to f32.  Lane l holds bins k = l + 64 q in registers.
//   magnitude mode: out[s][f][k]; bin k is contiguous, so lanes store directly
//   distance mode:  the x frame's magnitudes stay in registers while the y frame is transformed; three per-lane f64 sums
//                   (sum d^2 with d = y_mag - x_mag in f32, sum y_mag^2, sum |log y_mag - log x_mag| with correctly rounded
//                   f32 logs and their f32 difference); magnitudes are never written
//   mag distance:   the same three sums over two given magnitude tensors, grid-stride
//   shape distance: max |.| over windows of winlen samples of y_hat and of y, sum |a - b| (f32 difference, f64 sum)
// Every sum goes through reduce_f64.h: per-workgroup f64 partials in a caller-supplied slab (the workgroup count is a function
// of the shape only) and a one-wave finalize that folds them in a fixed order: no float atomics, bitwise reproducible run to run.
// Backward (adk_grad_stft_mag, adk_grad_stft_distance, adk_grad_shape_distance), with respect to the predicted signal only.  A
// frame's forward is recomputed by the same core, so the (re, im) walked back are the forward's own bits; the per-bin gradient of
// the magnitude becomes (g_re, g_im) = g (re, im) / mag where re^2 + im^2 >= eps, then stft_grad.h's tail (shared with mel.hip)
// and its gather.  The distance gradient reads the forward's folded sums and the upstream gradients from device memory: no host
// synchronisation.  The shape gradient puts one value at the first maximum of each window; windows are disjoint, so every
// sample is stored once.  No float atomics anywhere: bitwise reproducible.
#include "reduce_f64.h"
#include "stft_grad.h"

namespace adk {

constexpr int STFT_THREADS = FFT_WAVE;                 // one wave per workgroup
constexpr int STFT_MAX_WG = 2048;
constexpr int SHAPE_WAVE_WINLEN = 64;                  // winlen >= this: the 64 lanes of a wave share one window

template <int LOG2N>
__global__ __launch_bounds__(STFT_THREADS) void stft_mag_kernel(const float* __restrict__ x, int n_signals, StftFrameArgs a,
                                                                float* __restrict__ out) {
    constexpr int N = 1 << LOG2N, PER = FRAME_PER<LOG2N>;
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        float mag[PER];
        frame_spectrum<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw);
        frame_amplitudes<LOG2N>(buf, tw, a.eps, mag);
        float* o = out + (size_t)it * (N + 1);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int k = lane + q * STFT_THREADS;
            if (k <= N) o[k] = mag[q];
        }
    }
}

// log of an f32 rounded once: the f64 log, then one rounding.  The device logf is good to about 1 ulp; where few bins rise
// above the clamp (|log| = 8 there, 1 ulp = 9.5e-7) the sum of |dlog| over them inherits just that, several times the error of
// a correctly rounded log.
__device__ __forceinline__ float log_rounded(float v) { return (float)log((double)v); }

// The three terms of one (x_mag, y_mag) pair, added to the lane's sums.
__device__ __forceinline__ void stft_terms(float xm, float ym, double (&acc)[3]) {
    const float d = __fsub_rn(ym, xm);
    acc[0] += (double)d * (double)d;
    acc[1] += (double)ym * (double)ym;
    acc[2] += (double)fabsf(__fsub_rn(log_rounded(ym), log_rounded(xm)));
}

template <int LOG2N>
__global__ __launch_bounds__(STFT_THREADS) void stft_distance_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                     int n_signals, StftFrameArgs a, double* __restrict__ partial) {
    constexpr int N = 1 << LOG2N, PER = FRAME_PER<LOG2N>;
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        float xm[PER], ym[PER];
        frame_spectrum<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw);
        frame_amplitudes<LOG2N>(buf, tw, a.eps, xm);
        frame_spectrum<LOG2N>(y + (size_t)s * a.n_samples, f, a, buf, tw);
        frame_amplitudes<LOG2N>(buf, tw, a.eps, ym);
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (lane + q * STFT_THREADS <= N) stft_terms(xm[q], ym[q], acc);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double t = wave_sum(acc[j]);
        if (lane == 0) partial[3 * (size_t)blockIdx.x + j] = t;
    }
}

__global__ __launch_bounds__(RED_THREADS) void mag_distance_kernel(const float* __restrict__ x_mag, const float* __restrict__ y_mag,
                                                                  long long n, double* __restrict__ partial) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * RED_THREADS)
        stft_terms(x_mag[i], y_mag[i], acc);
    workgroup_partials<3>(acc, partial);
}

// max with MaxPool1d's NaN rule: a NaN in the window gives NaN
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// WAVE: one wave per (signal, window) item, lanes stride through the window and butterfly the max.  Otherwise one lane per item.
template <bool WAVE>
__global__ __launch_bounds__(RED_THREADS) void shape_distance_kernel(const float* __restrict__ y_hat, const float* __restrict__ y,
                                                                    int n_signals, int n_samples, int winlen,
                                                                    double* __restrict__ partial) {
    const long long windows = n_samples / winlen, items = windows * n_signals;
    double acc[1] = {0.0};
    if constexpr (WAVE) {
        const int lane = threadIdx.x & 63;
        for (long long it = (long long)blockIdx.x * RED_WAVES + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * RED_WAVES) {
            const long long s = it / windows, w = it - s * windows;
            const size_t base = (size_t)s * n_samples + (size_t)w * winlen;
            float ma = 0.f, mb = 0.f;
            for (int j = lane; j < winlen; j += 64) {
                ma = nan_max(ma, fabsf(y_hat[base + j]));
                mb = nan_max(mb, fabsf(y[base + j]));
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                ma = nan_max(ma, __shfl_xor(ma, off, 64));
                mb = nan_max(mb, __shfl_xor(mb, off, 64));
            }
            if (lane == 0) acc[0] += (double)fabsf(__fsub_rn(ma, mb));
        }
    } else {
        for (long long it = (long long)blockIdx.x * RED_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * RED_THREADS) {
            const long long s = it / windows, w = it - s * windows;
            const size_t base = (size_t)s * n_samples + (size_t)w * winlen;
            float ma = 0.f, mb = 0.f;
            for (int j = 0; j < winlen; ++j) {
                ma = nan_max(ma, fabsf(y_hat[base + j]));
                mb = nan_max(mb, fabsf(y[base + j]));
            }
            acc[0] += (double)fabsf(__fsub_rn(ma, mb));
        }
    }
    workgroup_partials<1>(acc, partial);
}

// ---- backward ----

__device__ __forceinline__ float sign_or_nan(float d) { return d > 0.f ? 1.f : d < 0.f ? -1.f : d; }   // sign(0) = 0, NaN stays NaN

// Windowed frame gradients of every frame into slab [n_signals][frames][n_fft]: the loop of stft_distance_kernel.  The gradient gX
// of magnitude bin k of the x frame is, DIST: c_sc (xm - ym) - c_mag sgn / xm with sgn the sign of the forward's own term
// log_rounded(ym) - log_rounded(xm), c_sc = scale_sc up_sc[0] / sqrt(S0 S1) (0 where S0 == 0: torch's norm backward at 0) and
// c_mag = scale_mag up_mag[0], both in f64 from device memory and rounded to f32, (S0, S1) = sums[0..1] as adk_stft_distance left
// them; else it is read from g [n_signals][frames][n_fft/2 + 1].
template <int LOG2N, bool DIST>
__global__ __launch_bounds__(STFT_THREADS) void stft_grad_frames_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                        const float* __restrict__ g, const double* __restrict__ sums,
                                                                        double scale_sc, const float* __restrict__ up_sc,
                                                                        double scale_mag, const float* __restrict__ up_mag,
                                                                        int n_signals, StftFrameArgs a, float* __restrict__ slab) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N, PER = FRAME_PER<LOG2N>;
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    float2* keep = reinterpret_cast<float2*>(FrameLds<LOG2N>::extra(lds));    // N + 1 bins
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    float c_sc = 0.f, c_mag = 0.f;
    if constexpr (DIST) {
        const double s0 = sums[0], s1 = sums[1];
        c_sc = s0 == 0.0 ? 0.f : (float)(scale_sc * (double)up_sc[0] / sqrt(s0 * s1));
        c_mag = (float)(scale_mag * (double)up_mag[0]);
    }
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        float xm[PER], gx[PER];
        if constexpr (DIST) {
            float ym[PER];
            frame_spectrum<LOG2N>(y + (size_t)s * a.n_samples, f, a, buf, tw);
            frame_amplitudes<LOG2N>(buf, tw, a.eps, ym);
            frame_spectrum<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw);
            frame_amplitudes<LOG2N, true>(buf, tw, a.eps, xm, keep);
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                gx[q] = 0.f;
                if (lane + q * STFT_THREADS <= N) {
                    const float sgn = sign_or_nan(__fsub_rn(log_rounded(ym[q]), log_rounded(xm[q])));
                    gx[q] = c_sc * __fsub_rn(xm[q], ym[q]) - c_mag * sgn / xm[q];
                }
            }
        } else {
            frame_spectrum<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw);
            frame_amplitudes<LOG2N, true>(buf, tw, a.eps, xm, keep);
            const float* gs = g + (size_t)it * (N + 1);
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int k = lane + q * STFT_THREADS;
                gx[q] = k <= N ? gs[k] : 0.f;
            }
        }
        // sqrt / clamp / power: (g_re, g_im) = gX (re, im) / mag; torch's clamp passes the gradient where re^2 + im^2 >= eps
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int k = lane + q * STFT_THREADS;
            if (k <= N) {
                const float2 c = keep[k];
                const float r = gx[q] / xm[q];
                keep[k] = c.x * c.x + c.y * c.y >= a.eps ? make_float2(r * c.x, r * c.y) : make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
        frame_grad_tail<LOG2N>(a, buf, tw, keep, slab + (size_t)it * NFFT);
    }
}

// The backward of shape_distance_kernel, in its two forms.  Per window: a = max |y_hat| and its FIRST index (what MaxPool1d's
// backward selects; the wave form reduces (value, index) pairs, a tie going to the lower index), b = max |y|;
// grad[index] = sign(a - b) sign(y_hat[index]) c, every other sample of the window and the dropped tail get 0.
template <bool WAVE>
__global__ __launch_bounds__(RED_THREADS) void shape_grad_kernel(const float* __restrict__ y_hat, const float* __restrict__ y,
                                                                int n_signals, int n_samples, int winlen, double scale,
                                                                const float* __restrict__ upstream, float* __restrict__ grad) {
    const long long windows = n_samples / winlen, items = windows * n_signals;
    const float c = (float)(scale * (double)upstream[0]);
    if constexpr (WAVE) {
        const int lane = threadIdx.x & 63;
        for (long long it = (long long)blockIdx.x * RED_WAVES + (threadIdx.x >> 6); it < items; it += (long long)gridDim.x * RED_WAVES) {
            const long long s = it / windows, w = it - s * windows;
            const size_t base = (size_t)s * n_samples + (size_t)w * winlen;
            float ma = 0.f, mb = 0.f;
            int idx = lane < winlen ? lane : 0;
            for (int j = lane; j < winlen; j += 64) {
                const float v = fabsf(y_hat[base + j]);
                if (v > ma || v != v) { ma = v; idx = j; }
                mb = nan_max(mb, fabsf(y[base + j]));
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(ma, off, 64);
                const int oi = __shfl_xor(idx, off, 64);
                if (ov > ma || (ov != ov && ma == ma) || (ov == ma && oi < idx)) { ma = ov; idx = oi; }
                mb = nan_max(mb, __shfl_xor(mb, off, 64));
            }
            ma = __shfl(ma, 0, 64);
            idx = __shfl(idx, 0, 64);
            const float v = sign_or_nan(__fsub_rn(ma, mb)) * sign_or_nan(y_hat[base + idx]) * c;
            for (int j = lane; j < winlen; j += 64) grad[base + j] = j == idx ? v : 0.f;
        }
    } else {
        for (long long it = (long long)blockIdx.x * RED_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * RED_THREADS) {
            const long long s = it / windows, w = it - s * windows;
            const size_t base = (size_t)s * n_samples + (size_t)w * winlen;
            float ma = 0.f, mb = 0.f;
            int idx = 0;
            for (int j = 0; j < winlen; ++j) {
                const float v = fabsf(y_hat[base + j]);
                if (v > ma || v != v) { ma = v; idx = j; }
                mb = nan_max(mb, fabsf(y[base + j]));
            }
            const float v = sign_or_nan(__fsub_rn(ma, mb)) * sign_or_nan(y_hat[base + idx]) * c;
            for (int j = 0; j < winlen; ++j) grad[base + j] = j == idx ? v : 0.f;
        }
    }
    // the tail MaxPool1d drops
    const long long tail = n_samples - windows * winlen, tails = tail * n_signals;
    for (long long e = (long long)blockIdx.x * RED_THREADS + threadIdx.x; e < tails; e += (long long)gridDim.x * RED_THREADS) {
        const long long s = e / tail, r = e - s * tail;
        grad[(size_t)s * n_samples + (size_t)(windows * winlen + r)] = 0.f;
    }
}

template <int LOG2N>
static void launch_stft_mag(const float* x, int n_signals, const StftFrameArgs& a, float* out, hipStream_t s) {
    const int n_wg = (int)std::min<long long>(a.frames * n_signals, 4 * STFT_MAX_WG);
    hipLaunchKernelGGL(stft_mag_kernel<LOG2N>, dim3(n_wg), dim3(STFT_THREADS), FrameLds<LOG2N>::bytes(), s, x, n_signals, a, out);
}

template <int LOG2N>
static void launch_stft_distance(const float* x, const float* y, int n_signals, const StftFrameArgs& a, int n_wg, double* partial,
                                 hipStream_t s) {
    hipLaunchKernelGGL(stft_distance_kernel<LOG2N>, dim3(n_wg), dim3(STFT_THREADS), FrameLds<LOG2N>::bytes(), s, x, y, n_signals, a,
                       partial);
}

static int mag_distance_workgroups(long long n) {
    return capped_workgroups((n + 4LL * RED_THREADS - 1) / (4LL * RED_THREADS), STFT_MAX_WG);
}

static int shape_workgroups(int n_signals, int n_samples, int winlen) {
    const long long items = (long long)(n_samples / winlen) * n_signals;
    const int per_wg = winlen >= SHAPE_WAVE_WINLEN ? RED_WAVES : RED_THREADS;
    return capped_workgroups((items + per_wg - 1) / per_wg, STFT_MAX_WG);
}

template <int LOG2N>
static size_t stft_grad_lds_bytes() { return FrameLds<LOG2N>::bytes(2 * ((1 << LOG2N) + 2)); }

template <int LOG2N>
static void launch_stft_grad_frames(const float* x, const float* y, const float* g, const double* sums, double scale_sc,
                                    const float* up_sc, double scale_mag, const float* up_mag, int n_signals, const StftFrameArgs& a,
                                    float* slab, hipStream_t s) {
    const int n_wg = capped_workgroups(a.frames * n_signals, STFT_MAX_WG);
    if (y)
        hipLaunchKernelGGL((stft_grad_frames_kernel<LOG2N, true>), dim3(n_wg), dim3(STFT_THREADS), stft_grad_lds_bytes<LOG2N>(), s,
                           x, y, g, sums, scale_sc, up_sc, scale_mag, up_mag, n_signals, a, slab);
    else
        hipLaunchKernelGGL((stft_grad_frames_kernel<LOG2N, false>), dim3(n_wg), dim3(STFT_THREADS), stft_grad_lds_bytes<LOG2N>(), s,
                           x, y, g, sums, scale_sc, up_sc, scale_mag, up_mag, n_signals, a, slab);
}

// Both STFT backward entry points: dist is the distance gradient (y, sums, scales, upstreams), else the VJP of g.
static int stft_grad(const char* fn, bool dist, const float* x, const float* y, const float* g, const double* sums, double scale_sc,
                     const float* up_sc, double scale_mag, const float* up_mag, int n_signals, int n_samples, int n_fft, int hop,
                     const float* window, int win_length, float eps, void* workspace, float* grad, void* stream) {
    const std::string f(fn);
    const int rc = check_stft_args(fn, n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    const bool given = dist ? (y && sums && up_sc && up_mag) : g != nullptr;
    if (n_signals > 0 && (!x || !given || !workspace || !grad)) return fail(ADK_ERR_ARG, f + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(g) |
         reinterpret_cast<uintptr_t>(up_sc) | reinterpret_cast<uintptr_t>(up_mag) | reinterpret_cast<uintptr_t>(workspace) |
         reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail(ADK_ERR_ARG, f + ": every pointer must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sums) & 7) return fail(ADK_ERR_ARG, f + ": sums must be 8-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad));
    const StftFrameArgs a(n_samples, n_fft, hop, window, win_length, eps);
    float* slab = static_cast<float*>(workspace);
    dispatch_log2n(n_fft, [&](auto L) {
        launch_stft_grad_frames<decltype(L)::value>(x, dist ? y : nullptr, g, sums, scale_sc, up_sc, scale_mag, up_mag, n_signals, a, slab, s);
    });
    ADK_HIP_CHECK(hipGetLastError());
    launch_frame_grad_gather(slab, n_signals, n_samples, 0, n_fft, hop, a.frames, grad, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_stft_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_stft_workspace_bytes: need n_signals >= 0, n_samples > 0, hop > 0, n_fft > 0");
    if (n_signals == 0) return 0;
    return (int64_t)capped_workgroups(stft_frames(n_samples, hop) * n_signals, STFT_MAX_WG) * 3 * (int64_t)sizeof(double);
}

extern "C" int adk_stft_mag(const float* x, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop, const float* window,
                            int32_t win_length, float eps, float* out, void* stream) {
    int rc = check_stft_args("adk_stft_mag", n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!x || !out)) return fail(ADK_ERR_ARG, "adk_stft_mag: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(ADK_ERR_ARG, "adk_stft_mag: x/out must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(out));
    const StftFrameArgs a(n_samples, n_fft, hop, window, win_length, eps);
    dispatch_log2n(n_fft, [&](auto L) { launch_stft_mag<decltype(L)::value>(x, n_signals, a, out, s); });
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_stft_distance(const float* x, const float* y, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                                 const float* window, int32_t win_length, float eps, double* sums, int64_t* count,
                                 void* workspace, float* sc, float* mag, void* stream) {
    int rc = check_stft_args("adk_stft_distance", n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    rc = check_accumulators("adk_stft_distance", sums, count, workspace, n_signals > 0, sc, mag);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!x || !y)) return fail(ADK_ERR_ARG, "adk_stft_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_stft_distance: x/y must be 4-byte aligned");
    if (n_signals == 0 && !sc && !mag) return ADK_OK;   // nothing to fold, nothing asked for
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sums));
    const StftFrameArgs a(n_samples, n_fft, hop, window, win_length, eps);
    const long long total = a.frames * n_signals;
    const int n_wg = n_signals > 0 ? capped_workgroups(total, STFT_MAX_WG) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n_signals > 0) {
        dispatch_log2n(n_fft, [&](auto L) { launch_stft_distance<decltype(L)::value>(x, y, n_signals, a, n_wg, partial, s); });
        ADK_HIP_CHECK(hipGetLastError());
    }
    launch_distance_finalize<3>(partial, n_wg, total * (long long)(n_fft / 2 + 1), sums, count, sc, mag, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int64_t adk_mag_distance_workspace_bytes(int64_t n) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_mag_distance_workspace_bytes: need n >= 0");
    if (n == 0) return 0;
    return (int64_t)mag_distance_workgroups(n) * 3 * (int64_t)sizeof(double);
}

extern "C" int adk_mag_distance(const float* x_mag, const float* y_mag, int64_t n, double* sums, int64_t* count, void* workspace,
                                float* sc, float* mag, void* stream) {
    if (n < 0) return fail(ADK_ERR_ARG, "adk_mag_distance: need n >= 0");
    int rc = check_accumulators("adk_mag_distance", sums, count, workspace, n > 0, sc, mag);
    if (rc != ADK_OK) return rc;
    if (n > 0 && (!x_mag || !y_mag)) return fail(ADK_ERR_ARG, "adk_mag_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(x_mag) | reinterpret_cast<uintptr_t>(y_mag)) & 3)
        return fail(ADK_ERR_ARG, "adk_mag_distance: x_mag/y_mag must be 4-byte aligned");
    if (n == 0 && !sc && !mag) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sums));
    const int n_wg = n > 0 ? mag_distance_workgroups(n) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n > 0) {
        hipLaunchKernelGGL(mag_distance_kernel, dim3(n_wg), dim3(RED_THREADS), 0, s, x_mag, y_mag, (long long)n, partial);
        ADK_HIP_CHECK(hipGetLastError());
    }
    launch_distance_finalize<3>(partial, n_wg, (long long)n, sums, count, sc, mag, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

static int check_shape(const char* fn, int n_signals, int n_samples, int winlen) {
    const std::string f(fn);
    if (n_signals < 0) return fail(ADK_ERR_ARG, f + ": need n_signals >= 0");
    if (winlen <= 0) return fail(ADK_ERR_ARG, f + ": need winlen > 0");
    if (n_samples < winlen) return fail(ADK_ERR_ARG, f + ": need n_samples >= winlen (MaxPool1d raises too)");
    return ADK_OK;
}

extern "C" int64_t adk_shape_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t winlen) {
    int rc = check_shape("adk_shape_workspace_bytes", n_signals, n_samples, winlen);
    if (rc != ADK_OK) return rc;
    if (n_signals == 0) return 0;
    return (int64_t)shape_workgroups(n_signals, n_samples, winlen) * (int64_t)sizeof(double);
}

extern "C" int adk_shape_distance(const float* y_hat, const float* y, int32_t n_signals, int32_t n_samples, int32_t winlen,
                                  double* sum, int64_t* count, void* workspace, float* loss, void* stream) {
    int rc = check_shape("adk_shape_distance", n_signals, n_samples, winlen);
    if (rc != ADK_OK) return rc;
    rc = check_accumulators("adk_shape_distance", sum, count, workspace, n_signals > 0, loss, nullptr);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!y_hat || !y)) return fail(ADK_ERR_ARG, "adk_shape_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(y_hat) | reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_shape_distance: y_hat/y must be 4-byte aligned");
    if (n_signals == 0 && !loss) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sum));
    const int n_wg = n_signals > 0 ? shape_workgroups(n_signals, n_samples, winlen) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n_signals > 0) {
        if (winlen >= SHAPE_WAVE_WINLEN)
            hipLaunchKernelGGL(shape_distance_kernel<true>, dim3(n_wg), dim3(RED_THREADS), 0, s, y_hat, y, n_signals, n_samples, winlen, partial);
        else
            hipLaunchKernelGGL(shape_distance_kernel<false>, dim3(n_wg), dim3(RED_THREADS), 0, s, y_hat, y, n_signals, n_samples, winlen, partial);
        ADK_HIP_CHECK(hipGetLastError());
    }
    launch_distance_finalize<1>(partial, n_wg, (long long)(n_samples / winlen) * n_signals, sum, count, nullptr, loss, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int64_t adk_grad_stft_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_grad_stft_workspace_bytes: need n_signals >= 0, n_samples > 0, hop > 0, n_fft > 0");
    return (int64_t)n_signals * stft_frames(n_samples, hop) * n_fft * (int64_t)sizeof(float);
}

extern "C" int adk_grad_stft_mag(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                                const float* window, int32_t win_length, float eps, void* workspace, float* grad_x, void* stream) {
    return stft_grad("adk_grad_stft_mag", false, x, nullptr, g, nullptr, 0.0, nullptr, 0.0, nullptr, n_signals, n_samples, n_fft, hop, window,
                     win_length, eps, workspace, grad_x, stream);
}

extern "C" int adk_grad_stft_distance(const float* x, const float* y, int32_t n_signals, int32_t n_samples, int32_t n_fft,
                                      int32_t hop, const float* window, int32_t win_length, float eps, const double* sums,
                                      double scale_sc, const float* up_sc, double scale_mag, const float* up_mag, void* workspace,
                                      float* grad_x, void* stream) {
    return stft_grad("adk_grad_stft_distance", true, x, y, nullptr, sums, scale_sc, up_sc, scale_mag, up_mag, n_signals, n_samples, n_fft,
                     hop, window, win_length, eps, workspace, grad_x, stream);
}

extern "C" int adk_grad_shape_distance(const float* y_hat, const float* y, int32_t n_signals, int32_t n_samples, int32_t winlen,
                                       double scale, const float* upstream, float* grad, void* stream) {
    int rc = check_shape("adk_grad_shape_distance", n_signals, n_samples, winlen);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!y_hat || !y || !upstream || !grad)) return fail(ADK_ERR_ARG, "adk_grad_shape_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(y_hat) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(upstream) |
         reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail(ADK_ERR_ARG, "adk_grad_shape_distance: every pointer must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad));
    const int n_wg = shape_workgroups(n_signals, n_samples, winlen);
    if (winlen >= SHAPE_WAVE_WINLEN)
        hipLaunchKernelGGL(shape_grad_kernel<true>, dim3(n_wg), dim3(RED_THREADS), 0, s, y_hat, y, n_signals, n_samples, winlen, scale, upstream, grad);
    else
        hipLaunchKernelGGL(shape_grad_kernel<false>, dim3(n_wg), dim3(RED_THREADS), 0, s, y_hat, y, n_signals, n_samples, winlen, scale, upstream, grad);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
