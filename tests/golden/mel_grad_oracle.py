"""Cases of tests/golden/mel_grad.npz and an fp64 NumPy restatement of the mel-spectrogram loss's backward.

``vjp64`` is the vector-Jacobian product of mel_oracle.logmel64 with respect to the waveform as torch's autograd defines it for
the reference's MelSpectrogram.forward (losses/mel_loss.py:84-94), step by step in float64:
  g_mel = g / (mel ln b) where the mel sum >= eps, else 0 (torch's clamp passes the gradient at equality);
  g_amp = g_mel @ melmat;   (g_re, g_im) = g_amp (re, im) / amp where re^2 + im^2 >= eps, else 0;
  g_frame[j] = sum_{k <= n_fft/2} g_re[k] cos(2 pi k j / n_fft) - g_im[k] sin(2 pi k j / n_fft)   (one-sided: no doubling);
  times the centred window, overlap-added into the padded signal, the reflect padding folded back onto the samples.
``loss_grad64`` is the gradient of MultiMelSpectrogramLoss.forward with respect to y_hat: per resolution the VJP of
g = sign(logmel(y_hat) - logmel(y)) / (count R), summed.  It takes the sign patterns to use instead of its own, so that a
float32 implementation, whose signs differ where the two log-mels are all but equal, is compared like with like.
It does not import the reference.
"""
import numpy as np

import mel_oracle as MO
from audiodec_amd import mel as _mel

G_SEED = 20240                                          # upstream gradients of the VJP cases: standard normal

# parameter sets: three of mel_oracle.PARAMS and three of this fixture's own
OWN_PARAMS = {
    "small": dict(fs=16000, fft_sizes=[256], hop_sizes=[32], win_lengths=[200], num_mels=40, fmin=0, fmax=8000, log_base=10.0),
    "big": dict(fs=48000, fft_sizes=[4096], hop_sizes=[1024], win_lengths=[4096], num_mels=128, fmin=0, fmax=24000,
                log_base=None),
    "gap": dict(fs=16000, fft_sizes=[256], hop_sizes=[300], win_lengths=[256], num_mels=40, fmin=0, fmax=8000, log_base=10.0),
}
CASES = [("vctk", (3, 1, 9600)), ("vctk", (2, 4500)), ("vctk", (2, 1, 7777)), ("vctk", (1, 1, 1025)),
         ("defaults", (2, 1, 7777)), ("defaults", (1, 1, 1025)),
         ("log2", (2, 4500)),
         ("small", (8, 1, 9600)), ("small", (2, 1, 129)),
         ("big", (1, 1, 6000)), ("big", (1, 1, 2049)),
         ("gap", (2, 1, 2000))]
STORE_MAX_SAMPLES = 16000                               # the reference's f32 gradients are stored for cases up to this size


def params(pname):
    if pname in OWN_PARAMS:
        p = dict(MO.DEFAULTS)
        p.update(OWN_PARAMS[pname])
        return p
    return MO.params(pname)


def key(pname, shape):
    return pname + "_" + "x".join(str(d) for d in shape)


def stored(shape):
    return int(np.prod(shape)) <= STORE_MAX_SAMPLES


def inputs(shape):
    """(y_hat, y) float32: y = mel_oracle._synth(shape, 100), y_hat = y + 0.01 noise as mel_oracle.inputs builds it."""
    y = MO._synth(shape, 100)
    noise = np.random.default_rng(MO.SEED + 7).standard_normal(shape).astype(np.float32)
    return (y + np.float32(0.01) * noise).astype(np.float32), y


def melmats(p):
    return [_mel.mel_filterbank(p["fs"], n_fft, p["num_mels"], p["fmin"], p["fmax"]) for n_fft, _, _ in MO.resolutions(p)]


def upstream(pname, shape, r, p):
    """The VJP case's upstream gradient (n, n_mels, frames) float32 for resolution r."""
    n = int(np.prod(shape[:-1]))
    _, hop, _ = MO.resolutions(p)[r]
    rng = np.random.default_rng([G_SEED, CASES.index((pname, tuple(shape))), r])
    return rng.standard_normal((n, p["num_mels"], 1 + shape[-1] // hop)).astype(np.float32)


def rel_l2(a, b):
    """||a - b|| / ||b|| in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def vjp64(x, g, n_fft, hop, win_length, melmat, eps=1e-10, log_base=None):
    """x (B, T) or (B, C, T), g (B*C, n_mels, frames) -> d sum(g * logmel64(x)) / dx, (B*C, T) float64."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        x = x.reshape(-1, x.shape[-1])
    n, T = x.shape
    half = n_fft // 2
    M = np.asarray(melmat, np.float64)
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = MO.hann_f32(win_length).astype(np.float64)
    xp = np.pad(x, ((0, 0), (half, half)), mode="reflect")
    frames = 1 + T // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(xp[:, idx] * w, axis=-1)                          # (n, frames, bins)
    power = spec.real ** 2 + spec.imag ** 2
    amp = np.sqrt(np.maximum(power, eps))
    mel = amp @ M.T                                                      # (n, frames, n_mels), unclamped
    lnb = 1.0 if log_base is None else np.log(log_base)
    gt = np.asarray(g, np.float64).transpose(0, 2, 1)
    g_mel = np.where(mel >= eps, gt / (np.maximum(mel, eps) * lnb), 0.0)
    g_amp = g_mel @ M
    r = np.where(power >= eps, g_amp / amp, 0.0)
    G = np.zeros((n, frames, n_fft), np.complex128)
    G[..., :half + 1] = r * spec                                         # g_re + i g_im
    g_frame = np.fft.ifft(G, axis=-1).real * n_fft * w                    # Re sum_k G[k] exp(+2 pi i k j / n_fft), windowed
    return overlap_add(g_frame, T, n_fft, hop)


def overlap_add(g_frame, T, n_fft, hop):
    """(n, frames, n_fft) frame values -> (n, T): summed into the padded signal, the reflect padding folded back."""
    n, frames, half = g_frame.shape[0], g_frame.shape[1], n_fft // 2
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    gp = np.zeros((n, T + 2 * half))
    np.add.at(gp, (np.arange(n)[:, None, None], idx[None]), g_frame)
    grad = gp[:, half:half + T].copy()
    grad[:, 1:half + 1] += gp[:, :half][:, ::-1]                          # padded u = -t
    grad[:, T - 1 - half:T - 1] += gp[:, half + T:][:, ::-1]              # padded u = 2 (T - 1) - t
    return grad


def coverage(T, n_fft, hop, win_length):
    """(T,) the sum of the centred window's weights over every frame position that maps to each sample: 0 exactly where no
    frame reaches the sample with a nonzero weight, which is where the gradient is an exact 0."""
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = MO.hann_f32(win_length).astype(np.float64)
    return overlap_add(np.broadcast_to(w, (1, 1 + T // hop, n_fft)), T, n_fft, hop)[0]


def signs64(y_hat, y, p, mms):
    """Per resolution: (sign(a - b), |a - b|) of the float64 log-mels."""
    out = []
    for (n_fft, hop, wl), mm in zip(MO.resolutions(p), mms):
        a = MO.logmel64(y_hat, p["fs"], n_fft, hop, wl, mm, p["eps"], p["log_base"])
        b = MO.logmel64(y, p["fs"], n_fft, hop, wl, mm, p["eps"], p["log_base"])
        out.append((np.sign(a - b), np.abs(a - b)))
    return out


def loss_grad64(y_hat, y, p, mms, signs=None):
    """d MultiMelSpectrogramLoss(y_hat, y) / d y_hat in float64, (n, T).  signs: one (n, n_mels, frames) array per resolution to
    use instead of sign(logmel64(y_hat) - logmel64(y))."""
    if signs is None:
        signs = [s for s, _ in signs64(y_hat, y, p, mms)]
    R = len(mms)
    total = 0.0
    for (n_fft, hop, wl), mm, s in zip(MO.resolutions(p), mms, signs):
        g = np.asarray(s, np.float64) / (s.size * R)
        total = total + vjp64(y_hat, g, n_fft, hop, wl, mm, p["eps"], p["log_base"])
    return total
