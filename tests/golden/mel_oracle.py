"""Cases of tests/golden/mel.npz and an fp64 NumPy restatement of the reference's mel-spectrogram loss (losses/mel_loss.py).

The restatement follows MelSpectrogram.forward step by step in float64: reflect padding of n_fft // 2, frames of n_fft every
hop samples, the float32 torch.hann_window centred in n_fft, a one-sided FFT, sqrt(max(power, eps)), the float32 filter bank
as given, max(., eps), the log; the loss is mean |a - b| per resolution, averaged over resolutions.  It is the yardstick both
the reference's float32 result and the HIP kernel are measured against.
"""
import numpy as np

from audiodec_amd import synth

SEED = 1337

# name: MultiMelSpectrogramLoss keyword arguments (the shipped configs' mel_loss_params, the class defaults, a log2 case)
PARAMS = {
    "vctk": dict(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048], window="hann_window", num_mels=80,
                 fmin=0, fmax=24000, log_base=None),
    "libritts": dict(fs=24000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048], window="hann_window", num_mels=80,
                     fmin=0, fmax=12000, log_base=None),
    "denoise": dict(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[None], window="hann_window", num_mels=80,
                    fmin=0, fmax=24000, log_base=None),
    "defaults": dict(),
    "log2": dict(fs=16000, fft_sizes=[512], hop_sizes=[128], win_lengths=[400], num_mels=64, fmin=80, fmax=7600, log_base=2.0),
}
DEFAULTS = dict(fs=22050, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240],
                window="hann_window", num_mels=80, fmin=80, fmax=7600, eps=1e-10, log_base=10.0)

# input name -> shape of y (y_hat has the same); "min" is (1, 1, max(fft_sizes) // 2 + 1)
INPUTS = ["synth3", "flat2", "odd", "min", "silence", "tiny", "full", "tone"]
SHAPES = {"synth3": (3, 1, 9600), "flat2": (2, 4500), "odd": (2, 1, 7777), "silence": (2, 1, 4800), "tiny": (2, 1, 4800),
          "full": (2, 1, 4800), "tone": (1, 1, 6000)}
# log-mels are stored for these (params, input) pairs (not all of them: size); losses for every pair
LOGMEL_CASES = {(p, i) for p in ("vctk", "libritts", "log2") for i in INPUTS if i != "synth3"} | {
    ("vctk", "synth3"), ("defaults", "flat2"), ("defaults", "min"), ("defaults", "silence"), ("denoise", "min")}


def params(name):
    p = dict(DEFAULTS)
    p.update(PARAMS[name])
    return p


def resolutions(p):
    return [(f, h, f if w is None else w) for f, h, w in zip(p["fft_sizes"], p["hop_sizes"], p["win_lengths"])]


def shape_of(pname, iname):
    if iname == "min":
        return (1, 1, max(params(pname)["fft_sizes"]) // 2 + 1)
    return SHAPES[iname]


def _synth(shape, base):
    n = int(np.prod(shape[:-1]))
    return np.stack([synth.synth_audio(SEED, base + s, shape[-1]) for s in range(n)]).reshape(shape).astype(np.float32)


def inputs(pname, iname):
    """(y_hat, y) float32 arrays of a case, regenerated from seeds."""
    shape = shape_of(pname, iname)
    y = _synth(shape, 100)
    noise = np.random.default_rng(SEED + 7).standard_normal(shape).astype(np.float32)
    y_hat = (y + np.float32(0.01) * noise).astype(np.float32)
    if iname == "silence":
        y_hat = np.zeros(shape, np.float32)
    elif iname == "tiny":
        y, y_hat = (y * np.float32(1e-4)).astype(np.float32), (y_hat * np.float32(1e-4)).astype(np.float32)
    elif iname == "full":
        y = np.where(y >= 0, np.float32(1), np.float32(-1)).astype(np.float32)
        y_hat = np.where(y_hat >= 0, np.float32(1), np.float32(-1)).astype(np.float32)
    elif iname == "tone":
        p = params(pname)
        n_fft = p["fft_sizes"][0]
        f = p["fs"] * 100.0 / n_fft                       # centre of bin 100 of the first resolution
        t = np.arange(shape[-1], dtype=np.float64) / p["fs"]
        y = (0.5 * np.sin(2 * np.pi * f * t)).astype(np.float32).reshape(shape)
        y_hat = (0.5 * np.sin(2 * np.pi * f * t + 0.3)).astype(np.float32).reshape(shape)
    return y_hat, y


def hann_f32(win_length):
    import torch
    return torch.hann_window(win_length).numpy()


def logmel64(x, fs_unused, n_fft, hop, win_length, melmat, eps=1e-10, log_base=None):
    """x (B, T) or (B, C, T) -> (B*C, n_mels, frames) float64.  melmat (n_mels, bins) as librosa returns it."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        x = x.reshape(-1, x.shape[-1])
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = hann_f32(win_length).astype(np.float64)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    frames = 1 + x.shape[-1] // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(xp[:, idx] * w, axis=-1)                 # (B, frames, bins)
    amp = np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, eps))
    mel = np.maximum(amp @ np.asarray(melmat, np.float64).T, eps)
    lg = np.log(mel) if log_base is None else np.log(mel) / np.log(log_base)
    return lg.transpose(0, 2, 1)


def loss64(y_hat, y, p, melmats):
    """MultiMelSpectrogramLoss.forward in float64; melmats: one (n_mels, bins) per resolution."""
    total = 0.0
    for (n_fft, hop, wl), mm in zip(resolutions(p), melmats):
        a = logmel64(y_hat, p["fs"], n_fft, hop, wl, mm, p["eps"], p["log_base"])
        b = logmel64(y, p["fs"], n_fft, hop, wl, mm, p["eps"], p["log_base"])
        total += float(np.mean(np.abs(a - b)))
    return total / len(melmats)
