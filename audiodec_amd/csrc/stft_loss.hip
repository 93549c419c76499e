// Multi-resolution STFT loss and waveform-shape loss (losses/stft_loss.py:19-170, losses/waveform_loss.py:15-75), one resolution
// or one window length per call.  The STFT is torch.stft's with its defaults (center=True, reflect padding of n_fft/2, one-sided,
// no normalisation, the window zero-padded to n_fft and centred):
//   frame f of signal s = x[s][f*hop - n_fft/2 + j] (reflected at both ends) * window_centred[j],   j < n_fft,  1 + T/hop frames
//   mag[k] = sqrt(clamp(re^2 + im^2, eps)),  k <= n_fft/2
// Organised as mel.hip: one frame is one wave64 workgroup, the frame lives in LDS, the FFT is fft_wave.h's, twiddles are built
// per workgroup in f64 and rounded to f32.  Lane l holds bins k = l + 64 q in registers.
//   magnitude mode: out[s][f][k]; bin k is contiguous, so lanes store directly
//   distance mode:  the x frame's magnitudes stay in registers while the y frame is transformed; three per-lane f64 sums
//                   (sum d^2 with d = y_mag - x_mag in f32, sum y_mag^2, sum |log y_mag - log x_mag| with correctly rounded
//                   f32 logs and their f32 difference); magnitudes are never written
//   mag distance:   the same three sums over two given magnitude tensors, grid-stride
//   shape distance: max |.| over windows of winlen samples of y_hat and of y, sum |a - b| (f32 difference, f64 sum)
// Every sum goes through per-workgroup f64 partials in a caller-supplied slab (the workgroup count is a function of the shape
// only) and a one-wave finalize that folds them in a fixed order: no float atomics, bitwise reproducible run to run.
#include "adk_common.h"
#include "fft_wave.h"

namespace adk {

constexpr int STFT_THREADS = FFT_WAVE;                 // one wave per workgroup
constexpr int STFT_MAX_WG = 2048;
constexpr int RED_THREADS = 256;                       // mag distance and shape distance: four waves per workgroup
constexpr int RED_WAVES = RED_THREADS / 64;
constexpr int SHAPE_WAVE_WINLEN = 64;                  // winlen >= this: the 64 lanes of a wave share one window

static long long stft_frames(int n_samples, int hop) { return 1 + (long long)n_samples / hop; }

static int capped_workgroups(long long items) {
    return (int)std::min<long long>(std::max<long long>(items, 1), STFT_MAX_WG);
}

struct StftArgs {
    int n_samples, hop, win_length, lpad;
    long long frames;
    float eps;
    const float* window;
};

// clamp(v, min=eps) as torch.clamp: NaN stays NaN
__device__ __forceinline__ float stft_clamp_min(float v, float eps) { return v < eps ? eps : v; }

// Magnitudes of frame f of signal x into mag[q] = bin lane + 64 q (0 past the last bin).  buf: n_fft floats of LDS.  Ends with a
// barrier, so the caller may reuse buf at once.
template <int LOG2N>
__device__ __forceinline__ void frame_mag(const float* __restrict__ x, long long f, const StftArgs& a, float* buf, const float2* tw,
                                          float (&mag)[((1 << LOG2N) + STFT_THREADS) / STFT_THREADS]) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N, HALF = NFFT / 2;
    constexpr int PER = (N + STFT_THREADS) / STFT_THREADS;
    const int lane = threadIdx.x;
    const long long t0 = f * a.hop - HALF;
    const int T = a.n_samples;
    // reflect padding and the centred zero-padded window at load time; sample j is float j of the complex buffer
#pragma unroll 4
    for (int j = lane; j < NFFT; j += STFT_THREADS) {
        long long t = t0 + j;
        t = t < 0 ? -t : t;
        t = t >= T ? 2LL * (T - 1) - t : t;
        const int jw = j - a.lpad;
        const float w = (jw >= 0 && jw < a.win_length) ? a.window[jw] : 0.f;
        buf[j] = __fmul_rn(x[t], w);
    }
    __syncthreads();
    float2* z = reinterpret_cast<float2*>(buf);
    wave_fft_dif<LOG2N>(z, tw);                                  // ends with a barrier
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int k = lane + q * STFT_THREADS;
        mag[q] = 0.f;
        if (k <= N) {
            float re, im;
            wave_fft_bin<LOG2N>(z, tw, k, re, im);
            mag[q] = sqrtf(stft_clamp_min(re * re + im * im, a.eps));
        }
    }
    __syncthreads();
}

template <int LOG2N>
__global__ __launch_bounds__(STFT_THREADS) void stft_mag_kernel(const float* __restrict__ x, int n_signals, StftArgs a,
                                                                float* __restrict__ out) {
    constexpr int N = 1 << LOG2N, PER = (N + STFT_THREADS) / STFT_THREADS;
    extern __shared__ float lds[];
    float2* tw = reinterpret_cast<float2*>(lds);                  // N + 1 twiddles
    float* buf = lds + 2 * (N + 2);                              // n_fft floats
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        float mag[PER];
        frame_mag<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw, mag);
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

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int LOG2N>
__global__ __launch_bounds__(STFT_THREADS) void stft_distance_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                     int n_signals, StftArgs a, double* __restrict__ partial) {
    constexpr int N = 1 << LOG2N, PER = (N + STFT_THREADS) / STFT_THREADS;
    extern __shared__ float lds[];
    float2* tw = reinterpret_cast<float2*>(lds);
    float* buf = lds + 2 * (N + 2);
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long s = it / a.frames, f = it - s * a.frames;
        float xm[PER], ym[PER];
        frame_mag<LOG2N>(x + (size_t)s * a.n_samples, f, a, buf, tw, xm);
        frame_mag<LOG2N>(y + (size_t)s * a.n_samples, f, a, buf, tw, ym);
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

// Sums of a four-wave workgroup in wave order into partial[NS * blockIdx.x ..].
template <int NS>
__device__ __forceinline__ void workgroup_partials(double (&acc)[NS], double* __restrict__ partial) {
    __shared__ double wsum[RED_WAVES][NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double t = wave_sum(acc[j]);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][j] = t;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = wsum[0][threadIdx.x];
        for (int w = 1; w < RED_WAVES; ++w) t += wsum[w][threadIdx.x];
        partial[NS * (size_t)blockIdx.x + threadIdx.x] = t;
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

// One wave: folds the slab into sums (workgroups in a fixed order) and adds count.  NS = 3: sc = sqrt(s0) / sqrt(s1) and
// mag = s2 / count from the totals; NS = 1: mag = s0 / count.  NaN on an empty total.
template <int NS>
__global__ __launch_bounds__(64) void distance_finalize_kernel(const double* __restrict__ partial, int n_wg, long long n_values,
                                                               double* __restrict__ sums, long long* __restrict__ count,
                                                               float* __restrict__ sc, float* __restrict__ mag) {
    const int lane = threadIdx.x;
    double t[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double v = 0.0;
        for (int b = lane; b < n_wg; b += 64) v += partial[NS * (size_t)b + j];
        t[j] = wave_sum(v);
    }
    if (lane == 0) {
        const long long n = count[0] + n_values;
        count[0] = n;
#pragma unroll
        for (int j = 0; j < NS; ++j) { t[j] += sums[j]; sums[j] = t[j]; }
        const float nan = __builtin_nanf("");
        if (sc) sc[0] = n > 0 ? (float)(sqrt(t[0]) / sqrt(t[NS > 1 ? 1 : 0])) : nan;
        if (mag) mag[0] = n > 0 ? (float)(t[NS - 1] / (double)n) : nan;
    }
}

template <int LOG2N>
static size_t stft_lds_bytes() {
    constexpr int N = 1 << LOG2N;
    return sizeof(float) * (2 * (N + 2) + 2 * N);
}

static int check_stft(const char* fn, int n_signals, int n_samples, int n_fft, int hop, const float* window, int win_length) {
    const std::string f(fn);
    if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return fail(ADK_ERR_ARG, f + ": n_fft must be a power of two in [256, 4096]");
    if (hop <= 0) return fail(ADK_ERR_ARG, f + ": need hop > 0");
    if (win_length <= 0 || win_length > n_fft) return fail(ADK_ERR_ARG, f + ": need 0 < win_length <= n_fft");
    if (n_signals < 0) return fail(ADK_ERR_ARG, f + ": need n_signals >= 0");
    if (n_samples <= n_fft / 2) return fail(ADK_ERR_ARG, f + ": reflect padding needs n_samples > n_fft / 2");
    if (!window) return fail(ADK_ERR_ARG, f + ": null pointer");
    if (reinterpret_cast<uintptr_t>(window) & 3) return fail(ADK_ERR_ARG, f + ": window must be 4-byte aligned");
    return ADK_OK;
}

// The accumulator, slab and result pointers every distance entry point takes.
static int check_accumulators(const char* fn, const void* sums, const void* count, const void* workspace, bool need_workspace,
                              const void* r0, const void* r1) {
    const std::string f(fn);
    if (!sums || !count) return fail(ADK_ERR_ARG, f + ": null accumulator pointer");
    if (need_workspace && !workspace) return fail(ADK_ERR_ARG, f + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(workspace)) & 7)
        return fail(ADK_ERR_ARG, f + ": sums/count/workspace must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(r1)) & 3)
        return fail(ADK_ERR_ARG, f + ": result pointers must be 4-byte aligned");
    return ADK_OK;
}

static StftArgs make_stft_args(int n_samples, int n_fft, int hop, const float* window, int win_length, float eps) {
    StftArgs a;
    a.n_samples = n_samples; a.hop = hop; a.win_length = win_length; a.lpad = (n_fft - win_length) / 2;
    a.frames = stft_frames(n_samples, hop); a.eps = eps; a.window = window;
    return a;
}

template <int LOG2N>
static void launch_stft_mag(const float* x, int n_signals, const StftArgs& a, float* out, hipStream_t s) {
    const int n_wg = (int)std::min<long long>(a.frames * n_signals, 4 * STFT_MAX_WG);
    hipLaunchKernelGGL(stft_mag_kernel<LOG2N>, dim3(n_wg), dim3(STFT_THREADS), stft_lds_bytes<LOG2N>(), s, x, n_signals, a, out);
}

template <int LOG2N>
static void launch_stft_distance(const float* x, const float* y, int n_signals, const StftArgs& a, int n_wg, double* partial,
                                 hipStream_t s) {
    hipLaunchKernelGGL(stft_distance_kernel<LOG2N>, dim3(n_wg), dim3(STFT_THREADS), stft_lds_bytes<LOG2N>(), s, x, y, n_signals, a,
                       partial);
}

static int stft_log2n(int n_fft) { int l = 0; while ((2 << l) < n_fft) ++l; return l; }

static int mag_distance_workgroups(long long n) { return capped_workgroups((n + 4LL * RED_THREADS - 1) / (4LL * RED_THREADS)); }

static int shape_workgroups(int n_signals, int n_samples, int winlen) {
    const long long items = (long long)(n_samples / winlen) * n_signals;
    const int per_wg = winlen >= SHAPE_WAVE_WINLEN ? RED_WAVES : RED_THREADS;
    return capped_workgroups((items + per_wg - 1) / per_wg);
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_stft_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_stft_workspace_bytes: need n_signals >= 0, n_samples > 0, hop > 0, n_fft > 0");
    if (n_signals == 0) return 0;
    return (int64_t)capped_workgroups(stft_frames(n_samples, hop) * n_signals) * 3 * (int64_t)sizeof(double);
}

extern "C" int adk_stft_mag(const float* x, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop, const float* window,
                            int32_t win_length, float eps, float* out, void* stream) {
    int rc = check_stft("adk_stft_mag", n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!x || !out)) return fail(ADK_ERR_ARG, "adk_stft_mag: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(ADK_ERR_ARG, "adk_stft_mag: x/out must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(out));
    const StftArgs a = make_stft_args(n_samples, n_fft, hop, window, win_length, eps);
    switch (stft_log2n(n_fft)) {
        case 7: launch_stft_mag<7>(x, n_signals, a, out, s); break;
        case 8: launch_stft_mag<8>(x, n_signals, a, out, s); break;
        case 9: launch_stft_mag<9>(x, n_signals, a, out, s); break;
        case 10: launch_stft_mag<10>(x, n_signals, a, out, s); break;
        default: launch_stft_mag<11>(x, n_signals, a, out, s); break;
    }
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_stft_distance(const float* x, const float* y, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                                 const float* window, int32_t win_length, float eps, double* sums, int64_t* count,
                                 void* workspace, float* sc, float* mag, void* stream) {
    int rc = check_stft("adk_stft_distance", n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    rc = check_accumulators("adk_stft_distance", sums, count, workspace, n_signals > 0, sc, mag);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!x || !y)) return fail(ADK_ERR_ARG, "adk_stft_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3)
        return fail(ADK_ERR_ARG, "adk_stft_distance: x/y must be 4-byte aligned");
    if (n_signals == 0 && !sc && !mag) return ADK_OK;   // nothing to fold, nothing asked for
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sums));
    const StftArgs a = make_stft_args(n_samples, n_fft, hop, window, win_length, eps);
    const long long total = a.frames * n_signals;
    const int n_wg = n_signals > 0 ? capped_workgroups(total) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n_signals > 0) {
        switch (stft_log2n(n_fft)) {
            case 7: launch_stft_distance<7>(x, y, n_signals, a, n_wg, partial, s); break;
            case 8: launch_stft_distance<8>(x, y, n_signals, a, n_wg, partial, s); break;
            case 9: launch_stft_distance<9>(x, y, n_signals, a, n_wg, partial, s); break;
            case 10: launch_stft_distance<10>(x, y, n_signals, a, n_wg, partial, s); break;
            default: launch_stft_distance<11>(x, y, n_signals, a, n_wg, partial, s); break;
        }
        ADK_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(distance_finalize_kernel<3>, dim3(1), dim3(64), 0, s, partial, n_wg, total * (long long)(n_fft / 2 + 1), sums,
                       reinterpret_cast<long long*>(count), sc, mag);
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
    hipLaunchKernelGGL(distance_finalize_kernel<3>, dim3(1), dim3(64), 0, s, partial, n_wg, (long long)n, sums,
                       reinterpret_cast<long long*>(count), sc, mag);
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
    hipLaunchKernelGGL(distance_finalize_kernel<1>, dim3(1), dim3(64), 0, s, partial, n_wg, (long long)(n_samples / winlen) * n_signals,
                       sum, reinterpret_cast<long long*>(count), static_cast<float*>(nullptr), loss);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}
