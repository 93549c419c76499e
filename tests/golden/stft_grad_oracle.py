"""Cases of tests/golden/stft_grad.npz and an fp64 NumPy restatement of the backward of the multi-resolution STFT loss and of the
waveform-shape loss.

``mag_vjp64`` is the vector-Jacobian product of stft_oracle.mag64 with respect to the waveform as torch's autograd defines it for
the reference's stft() (losses/stft_loss.py:19-35), step by step in float64:
  (g_re, g_im) = g (re, im) / mag where re^2 + im^2 >= eps, else 0 (torch's clamp passes the gradient at equality);
  g_frame[j] = sum_{k <= n_fft/2} g_re[k] cos(2 pi k j / n_fft) - g_im[k] sin(2 pi k j / n_fft)   (one-sided: no doubling);
  times the centred window, overlap-added into the padded signal, the reflect padding folded back onto the samples
  (mel_grad_oracle.overlap_add).
``res_grad64`` is the gradient with respect to x of  a_sc ||y_mag - x_mag||_F / ||y_mag||_F + a_mag mean |log y_mag - log x_mag|
for one resolution: the VJP of
  g = a_sc (x_mag - y_mag) / sqrt(S0 S1) - a_mag sgn / (count x_mag),   S0 = sum (y_mag - x_mag)^2,  S1 = sum y_mag^2,
  sgn = sign(log y_mag - log x_mag),  the first term 0 where S0 == 0 (torch's norm backward at 0);
``loss_grad64`` is the gradient of up_sc sc + up_mag mag of MultiResolutionSTFTLoss.forward: the sum over the R resolutions with
a_sc = up_sc / R and a_mag = up_mag / R.  Both take the sign patterns and the ``power >= eps`` masks to use instead of their own:
either is discontinuous, so a float32 implementation, whose signs and masks differ where the two log-magnitudes are all but equal
or the power all but eps, is compared like with like.
``shape_grad64`` is the gradient of MultiWindowShapeLoss.forward with respect to y_hat: per window length and window,
sign(max|y_hat| - max|y|) sign(y_hat[i]) / (R n windows) at the FIRST index i of the window's max |y_hat| (what torch's
max_pool1d backward selects), 0 elsewhere and in the dropped tail.
It does not import the reference.
"""
import numpy as np

import mel_grad_oracle as GO
import stft_oracle as SO
from mel_grad_oracle import coverage, inputs, overlap_add, rel_l2  # noqa: F401  (re-exported for the tests)

G_SEED = 20251                                          # upstream gradients of the VJP cases: standard normal
EPS = SO.EPS
WEAK_DLOG = 1e-4                                        # fp64 |log y_mag - log x_mag| below this: the sign is weak
WEAK_CAP = 0.01                                         # at most this fraction of a resolution's elements may be weak
FRAGILE_CAP = 8                                         # at most this many elements per resolution with power in [eps/2, 2 eps]

# parameter sets: stft_oracle.PARAMS and one of this fixture's own (hop > n_fft: some samples are covered by no frame)
OWN_PARAMS = {"gap": dict(fft_sizes=[256], hop_sizes=[300], win_lengths=[256], window="hann_window")}
CASES = [("defaults", (3, 1, 9600)), ("defaults", (2, 4500)), ("defaults", (1, 1, 1025)),
         ("edge", (1, 1, 6000)), ("edge", (1, 1, 2049)),
         ("hamming", (2, 1, 7777)), ("hamming", (2, 1, 257)),
         ("one", (2, 4500)),
         ("gap", (2, 1, 2000))]
STORE_MAX_SAMPLES = GO.STORE_MAX_SAMPLES                # the reference's f32 gradients are stored for cases up to this size

SHAPE_SHAPES = [(3, 1, 9600), (2, 1, 7777), (2, 4500)]                       # (2, 1, 7777) leaves a dropped tail
SHAPE_WNAMES = ["default", "w7", "w64", "w320", "whole"]
SHAPE_CASES = [(w, s) for w in SHAPE_WNAMES for s in SHAPE_SHAPES]
# the constructed cases: (2, 1, 2000) with window lengths [100, 7] (a wave per window and a lane per window)
BUILT_SHAPE, BUILT_WINLENS = (2, 1, 2000), [100, 7]
BUILT = ["tie", "equal"]


def params(pname):
    return OWN_PARAMS[pname] if pname in OWN_PARAMS else SO.PARAMS[pname]


def key(pname, shape):
    return pname + "_" + "x".join(str(d) for d in shape)


def stored(shape):
    return int(np.prod(shape)) <= STORE_MAX_SAMPLES


def windows_f32(p):
    return [SO.window_f32(p["window"], wl) for wl in p["win_lengths"]]


def upstream(pname, shape, r, p):
    """The VJP case's upstream gradient (n, frames, bins) float32 for resolution r."""
    n = int(np.prod(shape[:-1]))
    n_fft, hop, _ = SO.resolutions(p)[r]
    rng = np.random.default_rng([G_SEED, CASES.index((pname, tuple(shape))), r])
    return rng.standard_normal((n, 1 + shape[-1] // hop, n_fft // 2 + 1)).astype(np.float32)


def spectrum64(x, n_fft, hop, win_length, window):
    """x (B, T) or (B, C, T) -> (spec complex (n, frames, bins), the centred window (n_fft,), T), float64."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        x = x.reshape(-1, x.shape[-1])
    T = x.shape[-1]
    w = np.zeros(n_fft)
    lp = SO.left_pad(n_fft, win_length)
    w[lp:lp + win_length] = np.asarray(window, np.float64)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    idx = np.arange(SO.num_frames(T, hop))[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(xp[:, idx] * w, axis=-1), w, T


def power64(x, n_fft, hop, win_length, window):
    spec = spectrum64(x, n_fft, hop, win_length, window)[0]
    return spec.real ** 2 + spec.imag ** 2


def _vjp(spec, w, T, n_fft, hop, g, eps, mask):
    power = spec.real ** 2 + spec.imag ** 2
    mag = np.sqrt(np.maximum(power, eps))
    mask = power >= eps if mask is None else np.asarray(mask, bool)
    r = np.where(mask, np.asarray(g, np.float64) / mag, 0.0)
    G = np.zeros(spec.shape[:2] + (n_fft,), np.complex128)
    G[..., :n_fft // 2 + 1] = r * spec                                   # g_re + i g_im
    g_frame = np.fft.ifft(G, axis=-1).real * n_fft * w                    # Re sum_k G[k] exp(+2 pi i k j / n_fft), windowed
    return overlap_add(g_frame, T, n_fft, hop)


def mag_vjp64(x, g, n_fft, hop, win_length, window, eps=EPS, mask=None):
    """x (B, T) or (B, C, T), g (B*C, frames, bins) -> d sum(g * mag64(x)) / dx, (B*C, T) float64.  mask: the (B*C, frames, bins)
    pattern to use instead of power >= eps."""
    spec, w, T = spectrum64(x, n_fft, hop, win_length, window)
    return _vjp(spec, w, T, n_fft, hop, g, eps, mask)


def dlog64(x, y, p):
    """Per resolution: log y_mag - log x_mag of the float64 magnitudes."""
    return [np.log(SO.mag64(y, f, h, wl, win)) - np.log(SO.mag64(x, f, h, wl, win))
            for (f, h, wl), win in zip(SO.resolutions(p), windows_f32(p))]


def res_grad64(x, y, n_fft, hop, win_length, window, a_sc, a_mag, eps=EPS, sign=None, mask=None):
    """The gradient with respect to x of a_sc sc(x, y) + a_mag mag(x, y) for one resolution, (n, T) float64."""
    spec, w, T = spectrum64(x, n_fft, hop, win_length, window)
    xm = np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, eps))
    ym = SO.mag64(y, n_fft, hop, win_length, window, eps)
    s0, s1 = float(np.sum((ym - xm) ** 2)), float(np.sum(ym ** 2))
    sgn = np.sign(np.log(ym) - np.log(xm)) if sign is None else np.asarray(sign, np.float64)
    c_sc = 0.0 if s0 == 0.0 else a_sc / np.sqrt(s0 * s1)
    g = c_sc * (xm - ym) - (a_mag / xm.size) * sgn / xm
    return _vjp(spec, w, T, n_fft, hop, g, eps, mask)


def loss_grad64(x, y, p, up_sc, up_mag, signs=None, masks=None):
    """d (up_sc sc + up_mag mag) / dx of MultiResolutionSTFTLoss.forward in float64, (n, T).  signs, masks: one
    (n, frames, bins) array per resolution to use instead of sign(log y_mag - log x_mag) and power(x) >= eps."""
    R = len(p["fft_sizes"])
    total = 0.0
    for r, ((n_fft, hop, wl), win) in enumerate(zip(SO.resolutions(p), windows_f32(p))):
        total = total + res_grad64(x, y, n_fft, hop, wl, win, up_sc / R, up_mag / R, EPS,
                                   None if signs is None else signs[r], None if masks is None else masks[r])
    return total


# ---- waveform-shape loss ----

def built_inputs(name):
    """(y_hat, y) of a constructed case: inputs(BUILT_SHAPE) with planted samples of magnitude 2 (everything else is below 1).
    "tie": the same maximum twice in one window, once negative -- at (310, 350) of signal 0 (lanes 10 and 50 of window 3 of
    winlen 100), at (1210, 1274) (lane 10 twice), and at (700, 703) of signal 1 (one window of winlen 7).
    "equal": max|y_hat| == max|y| in the windows holding sample 310 of signal 0 (the same sample, opposite signs) and samples
    703 and 705 of signal 1."""
    y_hat, y = inputs(BUILT_SHAPE)
    y_hat, y = y_hat.copy(), y.copy()
    assert float(np.abs(y_hat).max()) < 1 and float(np.abs(y).max()) < 1
    if name == "tie":
        y_hat[0, 0, 310], y_hat[0, 0, 350] = -2.0, 2.0
        y_hat[0, 0, 1210], y_hat[0, 0, 1274] = 2.0, -2.0
        y_hat[1, 0, 700], y_hat[1, 0, 703] = 2.0, -2.0
    else:
        y_hat[0, 0, 310], y[0, 0, 310] = 2.0, -2.0
        y_hat[1, 0, 703], y[1, 0, 705] = -2.0, 2.0
    return y_hat, y


def shape_case(name, shape=None):
    """(y_hat, y, winlens) of a shape case: (window-list name, shape) or a constructed case's name."""
    if name in BUILT:
        return built_inputs(name) + (list(BUILT_WINLENS),)
    y_hat, y = inputs(shape)
    return y_hat, y, SO.shape_winlens(name, shape[-1])


def shape_key(name, shape=None):
    return "shape_" + (name if name in BUILT else key(name, shape))


def shape_maxima(y_hat, y, winlen):
    """(a, first index of a, b): max|y_hat|, its first index and max|y| per (signal, window)."""
    a, b = np.abs(np.asarray(y_hat, np.float64)), np.abs(np.asarray(y, np.float64))
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    n, nw = a.shape[0], a.shape[-1] // winlen
    a, b = a[:, :nw * winlen].reshape(n, nw, winlen), b[:, :nw * winlen].reshape(n, nw, winlen)
    return a.max(-1), a.argmax(-1), b.max(-1)                               # argmax returns the first


def shape_ties(y_hat, y, winlen):
    """(windows whose max|y_hat| occurs more than once, windows where max|y_hat| == max|y|)."""
    ma, _, mb = shape_maxima(y_hat, y, winlen)
    a = np.abs(np.asarray(y_hat, np.float64)).reshape(-1, np.shape(y_hat)[-1])
    nw = a.shape[-1] // winlen
    a = a[:, :nw * winlen].reshape(a.shape[0], nw, winlen)
    return int(((a == ma[..., None]).sum(-1) > 1).sum()), int((ma == mb).sum())


def shape_grad64(y_hat, y, winlens, up=1.0, magnitude=False):
    """d (up * MultiWindowShapeLoss(y_hat, y)) / d y_hat in float64, (n, T).  magnitude: the sum of the window lengths' terms'
    absolute values instead (what a float32 sum's rounding error scales with where terms of opposite sign meet at one sample)."""
    yh = np.asarray(y_hat, np.float64).reshape(-1, np.shape(y_hat)[-1])
    n, T = yh.shape
    grad = np.zeros((n, T))
    for w in winlens:
        ma, idx, mb = shape_maxima(y_hat, y, w)
        nw = T // w
        t = idx + np.arange(nw)[None, :] * w
        rows = np.arange(n)[:, None]
        term = np.sign(ma - mb) * np.sign(yh[rows, t]) * (up / (len(winlens) * n * nw))
        grad[rows, t] += np.abs(term) if magnitude else term
    return grad
