// The one-wave real FFT shared by mel.hip (log-mel and its backward), stft_loss.hip (STFT magnitudes), both through
// stft_frame.h, and univ_disc.hip (magnitude spectrogram and its backward).
// A frame of NFFT = 2 << LOG2N real samples lives in LDS as N = NFFT / 2 complex values and never leaves its wave: an N-point
// complex radix-2 decimation-in-frequency FFT (natural order in, bit-reversed order out) plus the even/odd untangle that reads
// the result back through the bit reversal.  Twiddles are exp(-2 pi i k / NFFT), k <= N, evaluated in f64 and rounded to f32.
// The callers are one-wave workgroups, so the barriers here are wave-local.
#pragma once
#include <hip/hip_runtime.h>

namespace adk {

constexpr int FFT_WAVE = 64;

template <int LOG2N>
__device__ void build_twiddles(float2* tw) {
    constexpr int NFFT = 2 << LOG2N, N = 1 << LOG2N;
    for (int k = threadIdx.x; k <= N; k += FFT_WAVE) {
        double s, c;
        sincospi(2.0 * (double)k / (double)NFFT, &s, &c);
        tw[k] = make_float2((float)c, (float)(-s));
    }
}

// In-place DIF over z[0 .. N): stage with half-span h pairs (i, i + h), twiddle exp(-2 pi i pos / 2h) = tw[pos * N / h].
// The caller has synchronised after filling z; ends with a barrier.
template <int LOG2N>
__device__ __forceinline__ void wave_fft_dif(float2* z, const float2* tw) {
    constexpr int N = 1 << LOG2N;
    const int lane = threadIdx.x;
#pragma unroll
    for (int lh = LOG2N - 1; lh >= 0; --lh) {
        const int h = 1 << lh;
#pragma unroll 4
        for (int b = lane; b < N / 2; b += FFT_WAVE) {
            const int pos = b & (h - 1);
            const int i = ((b - pos) << 1) + pos;
            const float2 u = z[i], v = z[i + h];
            const float2 w = tw[pos << (LOG2N - lh)];
            const float dx = u.x - v.x, dy = u.y - v.y;
            z[i] = make_float2(u.x + v.x, u.y + v.y);
            z[i + h] = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
        }
        __syncthreads();
    }
}

// Bin k <= N of the real FFT from the DIF result: X[k] = (Z[k] + conj Z[N-k]) / 2 + tw[k] (Z[k] - conj Z[N-k]) / 2i,
// Z[k] at its bit-reversed address.
template <int LOG2N>
__device__ __forceinline__ void wave_fft_bin(const float2* z, const float2* tw, int k, float& re, float& im) {
    constexpr int N = 1 << LOG2N;
    const int k1 = k & (N - 1), k2 = (N - k) & (N - 1);
    const float2 A = z[__builtin_bitreverse32((unsigned)k1) >> (32 - LOG2N)];
    const float2 B = z[__builtin_bitreverse32((unsigned)k2) >> (32 - LOG2N)];
    const float ex = 0.5f * (A.x + B.x), ey = 0.5f * (A.y - B.y);
    const float ox = 0.5f * (A.y + B.y), oy = -0.5f * (A.x - B.x);
    const float2 w = tw[k];
    re = ex + (ox * w.x - oy * w.y);
    im = ey + (ox * w.y + oy * w.x);
}

// The transposes (vector-Jacobian products) of the two steps above, for the backward of a spectrum-domain loss.  Both are the
// forward's linear maps transposed over the reals, with the forward's twiddles.

// Transpose of wave_fft_bin, gathered: the gradient of DIF result Z[p], p < N (natural index; the caller stores it at p's
// bit-reversed address), from the bin gradients g[k] = (d/d re, d/d im), k <= N.  Z[p] is operand A of bin p and operand B of bin
// N - p; Z[0] is both operands of bins 0 and N.  Summed in that fixed order.
template <int LOG2N>
__device__ __forceinline__ float2 wave_fft_bin_t(const float2* g, const float2* tw, int p) {
    constexpr int N = 1 << LOG2N;
    float gx = 0.f, gy = 0.f;
    auto add = [&](int k, bool as_a, bool as_b) {
        const float2 gk = g[k], w = tw[k];
        const float gox = gk.x * w.x + gk.y * w.y, goy = gk.y * w.x - gk.x * w.y;      // d/d ox, d/d oy
        if (as_a) { gx += 0.5f * (gk.x - goy); gy += 0.5f * (gk.y + gox); }
        if (as_b) { gx += 0.5f * (gk.x + goy); gy += 0.5f * (gox - gk.y); }
    };
    if (p == 0) {
        add(0, true, true);
        add(N, true, true);
    } else {
        add(p, true, false);
        add(N - p, false, true);
    }
    return make_float2(gx, gy);
}

// Transpose of wave_fft_dif: the DIF stages in reverse order, each transposed -- (u, v) <- (a + conj(w) c, a - conj(w) c) with
// the stage's own twiddle w -- which is a decimation-in-time FFT: bit-reversed order in, natural order out, in place.
// The caller has synchronised after filling z; ends with a barrier.
template <int LOG2N>
__device__ __forceinline__ void wave_fft_dit_t(float2* z, const float2* tw) {
    constexpr int N = 1 << LOG2N;
    const int lane = threadIdx.x;
#pragma unroll
    for (int lh = 0; lh < LOG2N; ++lh) {
        const int h = 1 << lh;
#pragma unroll 4
        for (int b = lane; b < N / 2; b += FFT_WAVE) {
            const int pos = b & (h - 1);
            const int i = ((b - pos) << 1) + pos;
            const float2 a = z[i], c = z[i + h];
            const float2 w = tw[pos << (LOG2N - lh)];
            const float tx = c.x * w.x + c.y * w.y, ty = c.y * w.x - c.x * w.y;
            z[i] = make_float2(a.x + tx, a.y + ty);
            z[i + h] = make_float2(a.x - tx, a.y - ty);
        }
        __syncthreads();
    }
}

}  // namespace adk
