"""Cases of tests/golden/stft_loss.npz and an fp64 NumPy restatement of the reference's multi-resolution STFT loss
(losses/stft_loss.py) and waveform-shape loss (losses/waveform_loss.py).

The restatement follows stft() step by step in float64, framed as mel_oracle.logmel64: reflect padding of n_fft // 2, frames of
n_fft every hop samples, the float32 torch window centred in n_fft with (n_fft - win_length) // 2 zeros on the left, a one-sided
FFT, sqrt(max(power, eps)).  x is the predicted signal, y the ground truth:  sc = ||y_mag - x_mag||_F / ||y_mag||_F,
mag = mean |log y_mag - log x_mag|, both averaged over resolutions.  The shape loss is mean |max|y_hat| - max|y|| over windows of
winlen samples (stride winlen, the tail dropped), averaged over window lengths.  It is the yardstick both the reference's
float32 result and the HIP kernels are measured against.
"""
import functools

import numpy as np

import mel_oracle as MO

# name: MultiResolutionSTFTLoss keyword arguments ("defaults" is every shipped config's stft_loss_params and the class defaults)
PARAMS = {
    "defaults": dict(fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window"),
    "one": dict(fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048], window="hann_window"),
    # 512/511: n_fft - win_length is odd, the left pad is floored
    "edge": dict(fft_sizes=[256, 512, 4096], hop_sizes=[64, 100, 1000], win_lengths=[200, 511, 4096], window="hann_window"),
    "hamming": dict(fft_sizes=[512], hop_sizes=[128], win_lengths=[400], window="hamming_window"),
}
EPS = 1e-7
TONE_FS = 48000.0

INPUTS = list(MO.INPUTS)                   # synth3, flat2, odd, min (T = max(fft) // 2 + 1), silence, tiny, full, tone
ORDINARY = ["synth3", "flat2", "odd", "min", "full", "silence"]
# the reference's magnitudes of y are stored for these (params, input) pairs (size); losses for every pair
MAG_CASES = [("defaults", "min"), ("one", "min"), ("edge", "min"), ("hamming", "min"), ("hamming", "tone"), ("hamming", "tiny")]

# name: MultiWindowShapeLoss winlen; None = one window of the whole signal, [T]
SHAPE_WINLENS = {"default": [300, 200, 100], "w300": [300], "w320": [320], "w7": [7], "whole": None, "w64": [64]}
SHAPE_INPUTS = ["synth3", "flat2", "odd", "silence", "tiny", "full"]          # odd: T = 7777 leaves a dropped tail


def resolutions(p):
    return list(zip(p["fft_sizes"], p["hop_sizes"], p["win_lengths"]))


def shape_of(pname, iname):
    if iname == "min":
        return (1, 1, max(PARAMS[pname]["fft_sizes"]) // 2 + 1)
    return MO.SHAPES[iname]


def inputs(pname, iname):
    """(x = y_hat, y) float32 arrays of a case, regenerated from seeds: mel_oracle's inputs, with "min" sized and "tone" placed
    (centre of bin 100 of the first resolution at 48 kHz) by this parameter set."""
    if iname not in ("min", "tone"):
        return MO.inputs("defaults", iname)
    shape = shape_of(pname, iname)
    if iname == "min":
        y = MO._synth(shape, 100)
        noise = np.random.default_rng(MO.SEED + 7).standard_normal(shape).astype(np.float32)
        return (y + np.float32(0.01) * noise).astype(np.float32), y
    f = TONE_FS * 100.0 / PARAMS[pname]["fft_sizes"][0]
    t = np.arange(shape[-1], dtype=np.float64) / TONE_FS
    y = (0.5 * np.sin(2 * np.pi * f * t)).astype(np.float32).reshape(shape)
    y_hat = (0.5 * np.sin(2 * np.pi * f * t + 0.3)).astype(np.float32).reshape(shape)
    return y_hat, y


def shape_winlens(wname, n_samples):
    w = SHAPE_WINLENS[wname]
    return [int(n_samples)] if w is None else list(w)


def window_f32(name, win_length):
    import torch
    return getattr(torch, name)(win_length).numpy().astype(np.float32)


def num_frames(n_samples, hop):
    return 1 + n_samples // hop


def left_pad(n_fft, win_length):
    return (n_fft - win_length) // 2


def mag64(x, n_fft, hop, win_length, window, eps=EPS):
    """x (B, T) or (B, C, T), window (win_length,) float32 values -> (B*C, frames, n_fft // 2 + 1) float64."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        x = x.reshape(-1, x.shape[-1])
    w = np.zeros(n_fft)
    lp = left_pad(n_fft, win_length)
    w[lp:lp + win_length] = np.asarray(window, np.float64)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    idx = np.arange(num_frames(x.shape[-1], hop))[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(xp[:, idx] * w, axis=-1)
    return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, eps))


def sc64(x_mag, y_mag):
    return float(np.sqrt(np.sum((y_mag - x_mag) ** 2)) / np.sqrt(np.sum(y_mag ** 2)))


def logmag64(x_mag, y_mag):
    return float(np.mean(np.abs(np.log(y_mag) - np.log(x_mag))))


def loss64(x, y, p):
    """MultiResolutionSTFTLoss.forward in float64 -> (sc, mag)."""
    sc = mag = 0.0
    for n_fft, hop, wl in resolutions(p):
        win = window_f32(p["window"], wl)
        xm, ym = mag64(x, n_fft, hop, wl, win), mag64(y, n_fft, hop, wl, win)
        sc += sc64(xm, ym)
        mag += logmag64(xm, ym)
    R = len(p["fft_sizes"])
    return sc / R, mag / R


@functools.lru_cache(maxsize=None)
def exact_loss(pname, iname):
    """fp64 (sc, mag) of a case, computed once per process and shared by the tests that need it."""
    return loss64(*inputs(pname, iname), PARAMS[pname])


def shape64(y_hat, y, winlens):
    """MultiWindowShapeLoss.forward in float64 (the float32 samples are exact in float64, so are the maxima)."""
    a, b = np.asarray(y_hat, np.float64), np.asarray(y, np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    total = 0.0
    for w in winlens:
        n = a.shape[-1] // w
        pa = np.abs(a[:, :n * w]).reshape(a.shape[0], n, w).max(-1)
        pb = np.abs(b[:, :n * w]).reshape(b.shape[0], n, w).max(-1)
        total += float(np.mean(np.abs(pa - pb)))
    return total / len(winlens)
