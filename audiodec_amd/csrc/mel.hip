// Log-mel spectrogram and mel L1 distance: MelSpectrogram.forward / MultiMelSpectrogramLoss.forward (losses/mel_loss.py:19-156)
// for one resolution, as torch.stft's defaults make it (center=True, reflect padding of n_fft/2, no normalisation, one-sided):
//   frame f of signal s = x[s][f*hop - n_fft/2 + j] (reflected at both ends) * window_centred[j],   j < n_fft,  1 + T/hop frames
//   amp[k] = sqrt(clamp(re^2 + im^2, eps)),  k <= n_fft/2;   mel[m] = clamp(sum_k amp[k] melmat[k][m], eps);   out = log(mel)
// One frame is one wave and never leaves it: the frame lives in LDS (n_fft floats = n_fft/2 complex), the n_fft-point real FFT
// is an n_fft/2-point complex radix-2 decimation-in-frequency FFT (natural order in, bit-reversed order out, read back through
// the bit reversal) plus the even/odd untangle.  Twiddles are exp(-2 pi i k / n_fft) evaluated in f64 and rounded to f32,
// built once per workgroup.  The mel filters come from a sparse table (one contiguous bin range per filter), summed in bin
// order.  A workgroup is one wave, so its barriers are wave-local; it loops over frames with no other synchronisation.
// The frame load, the FFT and the clamped amplitudes are stft_frame.h's (shared with stft_loss.hip).
//   logmel mode:   blocks of MEL_FB frames of one signal are staged in LDS, then stored as coalesced runs of (n_mels, frames)
//   distance mode: |logmel(a) - logmel(b)| in f32, summed per lane in f64, never stored; per-workgroup f64 partials in a slab
//                  and a fixed-order finalize launch (reduce_f64.h; no float atomics), so the sum is bitwise reproducible.
// Backward (adk_logmel_vjp, adk_mel_distance_grad): the vector-Jacobian product of the above with respect to the signal.  A frame's
// forward is recomputed (no spectra are saved), then walked back: log and clamp, the transposed mel projection (a sparse table per
// bin), sqrt/clamp/power, then stft_grad.h's tail (shared with stft_loss.hip): the transposed untangle and FFT, the window.  The
// windowed frame gradients go to a slab [n_signals][frames][n_fft]; a second launch gathers, per sample, its contributions through
// the reflect padding in ascending frame order: no float atomics, so the gradient is bitwise reproducible too.
#include "reduce_f64.h"
#include "stft_grad.h"

namespace adk {

constexpr int MEL_THREADS = FFT_WAVE;                  // one wave per workgroup
constexpr int MEL_MAX_MELS = 256;
constexpr int MEL_MPL = MEL_MAX_MELS / 64;             // mel filters per lane
constexpr int MEL_FB = 16;                             // logmel mode: frames per staged block
constexpr int MEL_MAX_WG = 2048;
constexpr int MEL_LOG_E = 0, MEL_LOG_2 = 2, MEL_LOG_10 = 10;

struct MelArgs : StftFrameArgs {
    int n_mels, n_weights, log_base;
    const int* fb_range;                               // [n_mels][3]: first bin, bin count, offset into fb_weight
    const float* fb_weight;
    MelArgs(int n_samples_, int n_fft, int hop_, const float* window_, int win_length_, const int32_t* fb_range_,
            const float* fb_weight_, int n_weights_, int n_mels_, int log_base_, float eps_)
        : StftFrameArgs(n_samples_, n_fft, hop_, window_, win_length_, eps_), n_mels(n_mels_), n_weights(n_weights_),
          log_base(log_base_), fb_range(reinterpret_cast<const int*>(fb_range_)), fb_weight(fb_weight_) {}
};

__device__ __forceinline__ float mel_log(float v, int base) {
    return base == MEL_LOG_10 ? log10f(v) : base == MEL_LOG_2 ? log2f(v) : logf(v);
}

// Log-mels of frame f of signal x into mels[i] = filter lane + 64 i.  buf: n_fft floats of LDS.  Ends with a barrier, so the
// caller may reuse buf at once.
// KEEP (the backward's recompute): also keep[k] = (re, im) of bin k <= N and sums[i] = the unclamped mel sum of mels[i]; buf[k]
// holds amp[k] on return.
template <int LOG2N, bool KEEP = false>
__device__ void frame_logmel(const float* __restrict__ x, long long f, const MelArgs& a, float* buf, const float2* tw,
                             float (&mels)[MEL_MPL], float2* keep = nullptr, float* sums = nullptr) {
    constexpr int N = 1 << LOG2N, PER = FRAME_PER<LOG2N>;
    const int lane = threadIdx.x;
    float amp[PER];
    frame_spectrum<LOG2N>(x, f, a, buf, tw);
    frame_amplitudes<LOG2N, KEEP>(buf, tw, a.eps, amp, keep);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int k = lane + q * MEL_THREADS;
        if (k <= N) buf[k] = amp[q];
    }
    __syncthreads();
    // mel filters: lane sums filter m = lane + 64 i over its bin range, in bin order
#pragma unroll
    for (int i = 0; i < MEL_MPL; ++i) {
        const int m = lane + i * MEL_THREADS;
        float s = 0.f;
        if (m < a.n_mels) {
            const int first = a.fb_range[3 * m], count = a.fb_range[3 * m + 1], off = a.fb_range[3 * m + 2];
            const int lo = max(first, 0), hi = off < 0 ? lo : min(min(first + count, N + 1), a.n_weights - off + first);
            for (int k = lo; k < hi; ++k) s = fmaf(a.fb_weight[off + (k - first)], buf[k], s);
        }
        mels[i] = mel_log(clamp_min(s, a.eps), a.log_base);
        if constexpr (KEEP) sums[i] = s;
    }
    __syncthreads();
}

template <int LOG2N>
__global__ __launch_bounds__(MEL_THREADS) void logmel_kernel(const float* __restrict__ x, int n_signals, MelArgs a,
                                                             float* __restrict__ out) {
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    float* stage = FrameLds<LOG2N>::extra(lds);                   // [n_mels][MEL_FB]
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long blocks = (a.frames + MEL_FB - 1) / MEL_FB;
    const long long items = blocks * n_signals;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int s = (int)(it / blocks);
        const long long f0 = (it - (long long)s * blocks) * MEL_FB;
        const int nb = (int)min((long long)MEL_FB, a.frames - f0);
        const float* xs = x + (size_t)s * a.n_samples;
        for (int j = 0; j < nb; ++j) {
            float mels[MEL_MPL];
            frame_logmel<LOG2N>(xs, f0 + j, a, buf, tw, mels);
#pragma unroll
            for (int i = 0; i < MEL_MPL; ++i) {
                const int m = lane + i * MEL_THREADS;
                if (m < a.n_mels) stage[m * MEL_FB + j] = mels[i];
            }
        }
        __syncthreads();
        float* os = out + (size_t)s * a.n_mels * a.frames + f0;
        for (int e = lane; e < a.n_mels * nb; e += MEL_THREADS) {
            const int m = e / nb, j = e - m * nb;
            os[(size_t)m * a.frames + j] = stage[m * MEL_FB + j];
        }
        __syncthreads();
    }
}

template <int LOG2N>
__global__ __launch_bounds__(MEL_THREADS) void mel_distance_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                   int n_signals, MelArgs a, double* __restrict__ partial) {
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    double acc = 0.0;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int s = (int)(it / a.frames);
        const long long f = it - (long long)s * a.frames;
        float ma[MEL_MPL], mb[MEL_MPL];
        frame_logmel<LOG2N>(xa + (size_t)s * a.n_samples, f, a, buf, tw, ma);
        frame_logmel<LOG2N>(xb + (size_t)s * a.n_samples, f, a, buf, tw, mb);
#pragma unroll
        for (int i = 0; i < MEL_MPL; ++i)
            if (lane + i * MEL_THREADS < a.n_mels) acc += (double)fabsf(__fsub_rn(ma[i], mb[i]));
    }
    acc = wave_sum(acc);
    if (lane == 0) partial[blockIdx.x] = acc;
}

// ---- backward ----
struct MelGradArgs {
    const int* tb_range;                               // [n_fft/2 + 1][3]: first filter, filter count, offset into tb_weight
    const float* tb_weight;
    int n_tweights;
};

// The VJP of frame_logmel for the frame it just ran on with KEEP (buf[k] = amp, keep[k] = (re, im), sums): g[i] is the gradient
// of log-mel lane + 64 i; out[j], j < n_fft, gets the windowed frame gradient.  gmel: MEL_MAX_MELS floats of LDS.  Ends with a
// barrier.
template <int LOG2N>
__device__ void frame_logmel_vjp(const MelArgs& a, const MelGradArgs& ga, float* buf, const float2* tw, float2* keep, float* gmel,
                                 const float (&sums)[MEL_MPL], const float (&g)[MEL_MPL], float* __restrict__ out) {
    constexpr int N = 1 << LOG2N, PER = FRAME_PER<LOG2N>;
    const int lane = threadIdx.x;
    // log and the second clamp: d log_b(mel) = 1 / (mel ln b); torch's clamp passes the gradient where mel >= eps
    const float lnb = a.log_base == MEL_LOG_10 ? 2.302585092994046f : a.log_base == MEL_LOG_2 ? 0.6931471805599453f : 1.f;
#pragma unroll
    for (int i = 0; i < MEL_MPL; ++i) {
        const int m = lane + i * MEL_THREADS;
        if (m < a.n_mels) gmel[m] = sums[i] >= a.eps ? g[i] / (sums[i] * lnb) : 0.f;
    }
    __syncthreads();
    // transposed mel projection in filter order, then sqrt / first clamp / power: (g_re, g_im) = g_amp (re, im) / amp
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int k = lane + q * MEL_THREADS;
        if (k <= N) {
            const int first = ga.tb_range[3 * k], count = ga.tb_range[3 * k + 1], off = ga.tb_range[3 * k + 2];
            const int lo = max(first, 0), hi = off < 0 ? lo : min(min(first + count, a.n_mels), ga.n_tweights - off + first);
            float s = 0.f;
            for (int m = lo; m < hi; ++m) s = fmaf(ga.tb_weight[off + (m - first)], gmel[m], s);
            const float2 c = keep[k];
            const float r = s / buf[k];
            keep[k] = c.x * c.x + c.y * c.y >= a.eps ? make_float2(r * c.x, r * c.y) : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    frame_grad_tail<LOG2N>(a, buf, tw, keep, out);
}

// Windowed frame gradients of every frame into slab [n_signals][frames][n_fft].  DIST: the upstream gradient of a frame's log-mels
// is sign(logmel(xa) - logmel(xb)) * (float)(scale * upstream[0]), the log-mels being the forward's own; else it is read from
// g [n_signals][n_mels][frames].
template <int LOG2N, bool DIST>
__global__ __launch_bounds__(MEL_THREADS) void mel_grad_frames_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                      const float* __restrict__ g, double scale,
                                                                      const float* __restrict__ upstream, int n_signals, MelArgs a,
                                                                      MelGradArgs ga, float* __restrict__ slab) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N;
    extern __shared__ float lds[];
    float2* tw = FrameLds<LOG2N>::tw(lds);
    float* buf = FrameLds<LOG2N>::buf(lds);
    float2* keep = reinterpret_cast<float2*>(FrameLds<LOG2N>::extra(lds));    // N + 1 bins
    float* gmel = FrameLds<LOG2N>::extra(lds) + 2 * (N + 2);     // MEL_MAX_MELS
    build_twiddles<LOG2N>(tw);
    __syncthreads();
    const int lane = threadIdx.x;
    const long long items = a.frames * n_signals;
    float c = 0.f;
    if constexpr (DIST) c = (float)(scale * (double)upstream[0]);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int s = (int)(it / a.frames);
        const long long f = it - (long long)s * a.frames;
        float ma[MEL_MPL], sums[MEL_MPL], gl[MEL_MPL];
        if constexpr (DIST) {
            float mb[MEL_MPL];
            frame_logmel<LOG2N>(xb + (size_t)s * a.n_samples, f, a, buf, tw, mb);
            frame_logmel<LOG2N, true>(xa + (size_t)s * a.n_samples, f, a, buf, tw, ma, keep, sums);
#pragma unroll
            for (int i = 0; i < MEL_MPL; ++i) {
                const float d = __fsub_rn(ma[i], mb[i]);
                gl[i] = d > 0.f ? c : d < 0.f ? -c : d;          // sign(0) = 0, NaN stays NaN
            }
        } else {
            frame_logmel<LOG2N, true>(xa + (size_t)s * a.n_samples, f, a, buf, tw, ma, keep, sums);
#pragma unroll
            for (int i = 0; i < MEL_MPL; ++i) {
                const int m = lane + i * MEL_THREADS;
                gl[i] = m < a.n_mels ? g[((size_t)s * a.n_mels + m) * a.frames + f] : 0.f;
            }
        }
        frame_logmel_vjp<LOG2N>(a, ga, buf, tw, keep, gmel, sums, gl, slab + (size_t)it * NFFT);
    }
}

template <int LOG2N>
static size_t mel_grad_lds_bytes() { return FrameLds<LOG2N>::bytes(2 * ((1 << LOG2N) + 2) + MEL_MAX_MELS); }

static int check_common(const char* fn, int n_signals, int n_samples, int n_fft, int hop, const float* window, int win_length,
                        const int32_t* fb_range, const float* fb_weight, int n_weights, int n_mels, int log_base) {
    const std::string f(fn);
    const int rc = check_stft_args(fn, n_signals, n_samples, n_fft, hop, window, win_length);
    if (rc != ADK_OK) return rc;
    if (n_mels <= 0 || n_mels > MEL_MAX_MELS) return fail(ADK_ERR_ARG, f + ": need 0 < n_mels <= 256");
    if (n_weights <= 0) return fail(ADK_ERR_ARG, f + ": need n_weights > 0");
    if (log_base != MEL_LOG_E && log_base != MEL_LOG_2 && log_base != MEL_LOG_10)
        return fail(ADK_ERR_ARG, f + ": log_base must be 0 (natural), 2 or 10");
    if (!fb_range || !fb_weight) return fail(ADK_ERR_ARG, f + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(fb_range) | reinterpret_cast<uintptr_t>(fb_weight)) & 3)
        return fail(ADK_ERR_ARG, f + ": fb_range/fb_weight must be 4-byte aligned");
    return ADK_OK;
}

template <int LOG2N>
static void launch_logmel(const float* x, int n_signals, const MelArgs& a, float* out, hipStream_t s) {
    const long long items = (a.frames + MEL_FB - 1) / MEL_FB * n_signals;
    const int n_wg = (int)std::min<long long>(items, 4 * MEL_MAX_WG);
    hipLaunchKernelGGL(logmel_kernel<LOG2N>, dim3(n_wg), dim3(MEL_THREADS), FrameLds<LOG2N>::bytes((size_t)a.n_mels * MEL_FB), s, x, n_signals, a, out);
}

template <int LOG2N>
static void launch_distance(const float* xa, const float* xb, int n_signals, const MelArgs& a, int n_wg, double* partial, hipStream_t s) {
    hipLaunchKernelGGL(mel_distance_kernel<LOG2N>, dim3(n_wg), dim3(MEL_THREADS), FrameLds<LOG2N>::bytes(), s,
                       xa, xb, n_signals, a, partial);
}

template <int LOG2N>
static void launch_grad_frames(const float* xa, const float* xb, const float* g, double scale, const float* upstream, int n_signals,
                               const MelArgs& a, const MelGradArgs& ga, float* slab, hipStream_t s) {
    const int n_wg = capped_workgroups(a.frames * n_signals, MEL_MAX_WG);
    if (xb)
        hipLaunchKernelGGL((mel_grad_frames_kernel<LOG2N, true>), dim3(n_wg), dim3(MEL_THREADS), mel_grad_lds_bytes<LOG2N>(), s,
                           xa, xb, g, scale, upstream, n_signals, a, ga, slab);
    else
        hipLaunchKernelGGL((mel_grad_frames_kernel<LOG2N, false>), dim3(n_wg), dim3(MEL_THREADS), mel_grad_lds_bytes<LOG2N>(), s,
                           xa, xb, g, scale, upstream, n_signals, a, ga, slab);
}

// Both backward entry points: xb != nullptr is the distance gradient (scale, upstream), else the VJP of g.
static int mel_grad(const char* fn, const float* xa, const float* xb, const float* g, double scale, const float* upstream,
                    int n_signals, int n_samples, int n_fft, int hop, const float* window, int win_length, const int32_t* fb_range,
                    const float* fb_weight, int n_weights, int n_mels, int log_base, float eps, const int32_t* tb_range,
                    const float* tb_weight, int n_tweights, void* workspace, float* grad, void* stream) {
    const std::string f(fn);
    int rc = check_common(fn, n_signals, n_samples, n_fft, hop, window, win_length, fb_range, fb_weight, n_weights, n_mels, log_base);
    if (rc != ADK_OK) return rc;
    if (n_tweights <= 0) return fail(ADK_ERR_ARG, f + ": need n_tweights > 0");
    if (!tb_range || !tb_weight) return fail(ADK_ERR_ARG, f + ": null pointer");
    if (n_signals > 0 && (!xa || !(xb ? (const void*)upstream : (const void*)g) || !workspace || !grad))
        return fail(ADK_ERR_ARG, f + ": null pointer");
    if ((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(g) |
         reinterpret_cast<uintptr_t>(upstream) | reinterpret_cast<uintptr_t>(tb_range) | reinterpret_cast<uintptr_t>(tb_weight) |
         reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail(ADK_ERR_ARG, f + ": every pointer must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(grad));
    const MelArgs a(n_samples, n_fft, hop, window, win_length, fb_range, fb_weight, n_weights, n_mels, log_base, eps);
    MelGradArgs ga;
    ga.tb_range = reinterpret_cast<const int*>(tb_range); ga.tb_weight = tb_weight; ga.n_tweights = n_tweights;
    float* slab = static_cast<float*>(workspace);
    dispatch_log2n(n_fft, [&](auto L) {
        launch_grad_frames<decltype(L)::value>(xa, xb, g, scale, upstream, n_signals, a, ga, slab, s);
    });
    ADK_HIP_CHECK(hipGetLastError());
    launch_frame_grad_gather(slab, n_signals, n_samples, 0, n_fft, hop, a.frames, grad, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

}  // namespace adk

using namespace adk;

extern "C" int64_t adk_mel_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_mel_workspace_bytes: need n_signals >= 0, n_samples > 0, hop > 0, n_fft > 0");
    if (n_signals == 0) return 0;
    return (int64_t)capped_workgroups(stft_frames(n_samples, hop) * n_signals, MEL_MAX_WG) * (int64_t)sizeof(double);
}

extern "C" int adk_logmel(const float* x, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop, const float* window,
                          int32_t win_length, const int32_t* fb_range, const float* fb_weight, int32_t n_weights, int32_t n_mels,
                          int32_t log_base, float eps, float* out, void* stream) {
    int rc = check_common("adk_logmel", n_signals, n_samples, n_fft, hop, window, win_length, fb_range, fb_weight, n_weights,
                          n_mels, log_base);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!x || !out)) return fail(ADK_ERR_ARG, "adk_logmel: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(ADK_ERR_ARG, "adk_logmel: x/out must be 4-byte aligned");
    if (n_signals == 0) return ADK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(out));
    const MelArgs a(n_samples, n_fft, hop, window, win_length, fb_range, fb_weight, n_weights, n_mels, log_base, eps);
    dispatch_log2n(n_fft, [&](auto L) { launch_logmel<decltype(L)::value>(x, n_signals, a, out, s); });
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int adk_mel_distance(const float* a_sig, const float* b_sig, int32_t n_signals, int32_t n_samples, int32_t n_fft,
                                int32_t hop, const float* window, int32_t win_length, const int32_t* fb_range,
                                const float* fb_weight, int32_t n_weights, int32_t n_mels, int32_t log_base, float eps,
                                double* sum, int64_t* count, void* workspace, float* loss, void* stream) {
    int rc = check_common("adk_mel_distance", n_signals, n_samples, n_fft, hop, window, win_length, fb_range, fb_weight,
                          n_weights, n_mels, log_base);
    if (rc != ADK_OK) return rc;
    rc = check_accumulators("adk_mel_distance", sum, count, workspace, n_signals > 0, loss, nullptr);
    if (rc != ADK_OK) return rc;
    if (n_signals > 0 && (!a_sig || !b_sig)) return fail(ADK_ERR_ARG, "adk_mel_distance: null pointer");
    if ((reinterpret_cast<uintptr_t>(a_sig) | reinterpret_cast<uintptr_t>(b_sig)) & 3)
        return fail(ADK_ERR_ARG, "adk_mel_distance: a/b must be 4-byte aligned");
    if (n_signals == 0 && !loss) return ADK_OK;        // nothing to fold, nothing asked for
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(device_of(sum));
    const MelArgs a(n_samples, n_fft, hop, window, win_length, fb_range, fb_weight, n_weights, n_mels, log_base, eps);
    const long long total = a.frames * n_signals;
    const int n_wg = n_signals > 0 ? capped_workgroups(total, MEL_MAX_WG) : 0;
    double* partial = static_cast<double*>(workspace);
    if (n_signals > 0) {
        dispatch_log2n(n_fft, [&](auto L) { launch_distance<decltype(L)::value>(a_sig, b_sig, n_signals, a, n_wg, partial, s); });
        ADK_HIP_CHECK(hipGetLastError());
    }
    launch_distance_finalize<1>(partial, n_wg, total * (long long)n_mels, sum, count, nullptr, loss, s);
    ADK_HIP_CHECK(hipGetLastError());
    return ADK_OK;
}

extern "C" int64_t adk_mel_grad_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop) {
    if (n_signals < 0 || n_samples <= 0 || hop <= 0 || n_fft <= 0)
        return fail(ADK_ERR_ARG, "adk_mel_grad_workspace_bytes: need n_signals >= 0, n_samples > 0, hop > 0, n_fft > 0");
    return (int64_t)n_signals * stft_frames(n_samples, hop) * n_fft * (int64_t)sizeof(float);
}

extern "C" int adk_logmel_vjp(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                              const float* window, int32_t win_length, const int32_t* fb_range, const float* fb_weight,
                              int32_t n_weights, int32_t n_mels, int32_t log_base, float eps, const int32_t* tb_range,
                              const float* tb_weight, int32_t n_tweights, void* workspace, float* grad_x, void* stream) {
    return mel_grad("adk_logmel_vjp", x, nullptr, g, 0.0, nullptr, n_signals, n_samples, n_fft, hop, window, win_length, fb_range,
                    fb_weight, n_weights, n_mels, log_base, eps, tb_range, tb_weight, n_tweights, workspace, grad_x, stream);
}

extern "C" int adk_mel_distance_grad(const float* a_sig, const float* b_sig, int32_t n_signals, int32_t n_samples, int32_t n_fft,
                                     int32_t hop, const float* window, int32_t win_length, const int32_t* fb_range,
                                     const float* fb_weight, int32_t n_weights, int32_t n_mels, int32_t log_base, float eps,
                                     const int32_t* tb_range, const float* tb_weight, int32_t n_tweights, double scale,
                                     const float* upstream, void* workspace, float* grad_a, void* stream) {
    if (n_signals > 0 && !b_sig) return fail(ADK_ERR_ARG, "adk_mel_distance_grad: null pointer");
    return mel_grad("adk_mel_distance_grad", a_sig, b_sig, nullptr, scale, upstream, n_signals, n_samples, n_fft, hop, window,
                    win_length, fb_range, fb_weight, n_weights, n_mels, log_base, eps, tb_range, tb_weight, n_tweights, workspace,
                    grad_a, stream);
}
