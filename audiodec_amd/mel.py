"""Mel-spectrogram loss on the device: the reference's evaluation metric (adk_logmel, adk_mel_distance).

Mirrors ``losses/mel_loss.py``: ``MelSpectrogram`` (lines 19-94) and ``MultiMelSpectrogramLoss`` (lines 97-156), which the
reference's trainers build from ``config['mel_loss_params']`` (codecTrain.py:202-205) and use as the metric loss
(trainer/trainerGAN.py:214-241).  Every shipped config enables it (``use_mel_loss: true``) and nothing else of the metric.

The filter bank is ``librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)`` with librosa's defaults (Slaney mel scale, Slaney
area normalisation, float32), restated here in NumPy; librosa is not a dependency.  Each resolution runs one HIP kernel:
framing with reflect padding, an n_fft-point real FFT, the mel projection from a sparse filter table, the log and -- for the
loss -- the L1 sum, folded into an f64 accumulator on the device without ever writing the log-mels.

Forward only by default: an input that requires grad while grad is enabled raises NotImplementedError.  Built with
``differentiable=True``, ``MelSpectrogram`` and ``MultiMelSpectrogramLoss`` give the waveform (the loss: the generated signal
``y_hat`` only) a gradient through ``torch.autograd`` (adk_logmel_vjp, adk_mel_distance_grad): each frame's forward is
recomputed and walked back on the device, and the frame gradients are overlap-added in a fixed order, so the gradient is
bitwise reproducible like the value.  The backward is once-differentiable.
"""
import math

import numpy as np
import torch

from . import lazy_guard, native
from .loss_common import (_Accumulator, _check_fft_size, _check_length, _mean_f32, _no_grad_inputs, _ptr, _settled, _signals,
                          _wants_grad, _workspace, num_frames)

_LOG_BASES = {None: 0, 2.0: 2, 10.0: 10}


# ---- librosa.filters.mel with its defaults (htk=False, norm='slaney', dtype=float32) ----
def hz_to_mel(freq):
    """Slaney mel scale: linear below 1 kHz (200/3 Hz per mel), logarithmic above (1000 Hz = 15 mel, step ln(6.4)/27)."""
    f = np.asarray(freq, np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(mels):
    m = np.asarray(mels, np.float64)
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """(n_mels, 1 + n_fft // 2) float32: the triangles are computed in f64 and stored into a float32 array, then scaled by the
    f64 Slaney norm 2 / (f[m+2] - f[m]) in place, as librosa does."""
    fmax = sr / 2.0 if fmax is None else fmax
    weights = np.zeros((n_mels, 1 + n_fft // 2), np.float32)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


def sparse_filters(melmat):
    """(n_mels, bins) -> (range int32 [n_mels][3] = first bin, count, offset; weights float32): one contiguous bin range per
    filter, from its first to its last nonzero weight (zeros inside the range are kept)."""
    rng, ws, off = [], [], 0
    for row in np.asarray(melmat, np.float32):
        nz = np.nonzero(row)[0]
        first, count = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        rng.append((first, count, off))
        ws.append(row[first:first + count])
        off += count
    w = np.concatenate(ws) if off else np.zeros(1, np.float32)
    return np.asarray(rng, np.int32), np.ascontiguousarray(w, np.float32)


def transposed_filters(melmat):
    """(n_mels, bins) -> (range int32 [bins][3] = first filter, count, offset; weights float32): sparse_filters of melmat.T, one
    contiguous filter range per bin, for the backward's g_amp[k] = sum_m melmat[m][k] g_mel[m]."""
    return sparse_filters(np.ascontiguousarray(np.asarray(melmat, np.float32).T))


def _grad_workspace(n, T, n_fft, hop, dev):
    ws_bytes = int(native.lib().adk_mel_grad_workspace_bytes(n, T, n_fft, hop))
    if ws_bytes < 0:
        native.check(ws_bytes, "adk_mel_grad_workspace_bytes")
    return torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)


class _LogMelFn(torch.autograd.Function):
    """MelSpectrogram.forward with a backward: adk_logmel, and adk_logmel_vjp on the saved signal."""

    @staticmethod
    def forward(ctx, x, mel):
        xs = _signals(x.detach(), mel._dev)
        ctx.mel, ctx.like = mel, (x.shape, x.device, x.dtype)
        ctx.save_for_backward(xs)
        return mel._logmel(xs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (xs,), mel, (shape, device, dtype) = ctx.saved_tensors, ctx.mel, ctx.like
        grad = mel._vjp(xs, g.to(dtype=torch.float32).contiguous())
        return grad.reshape(shape).to(device=device, dtype=dtype), None


class _MelLossFn(torch.autograd.Function):
    """MultiMelSpectrogramLoss.forward with a backward with respect to y_hat: the fold path's value, and per resolution
    adk_mel_distance_grad with scale 1 / (count R), summed over the resolutions in their order."""

    @staticmethod
    def forward(ctx, y_hat, loss, a, b):
        ctx.loss, ctx.like = loss, (y_hat.shape, y_hat.device, y_hat.dtype)
        ctx.save_for_backward(a, b)
        return loss._value(a, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (a, b), loss, (shape, device, dtype) = ctx.saved_tensors, ctx.loss, ctx.like
        up = g.to(dtype=torch.float32).reshape(1).contiguous()
        R = len(loss.mel_transfers)
        grad = None
        for f in loss.mel_transfers:
            count = a.shape[0] * f.num_mels * f.num_frames(a.shape[1])
            gr = f._distance_grad(a, b, 1.0 / (float(count) * R), up)
            grad = gr if grad is None else grad + gr
        return grad.reshape(shape).to(device=device, dtype=dtype), None, None, None


class MelSpectrogram:
    """losses/mel_loss.py:19-94 on the HIP path.  Same arguments and defaults.

    As in the reference, ``center``, ``normalized`` and ``onesided`` are accepted and stored but IGNORED: its torch.stft call
    passes none of them, so torch's defaults always apply -- center=True with reflect padding of fft_size // 2, no
    normalisation, a one-sided spectrum.  Reflect padding needs T > fft_size // 2 (torch raises otherwise; so does this).
    Only ``window="hann_window"`` and power-of-two ``fft_size`` in [256, 4096] are implemented.
    ``differentiable=True`` (not in the reference, whose modules always are): an ``x`` that requires grad gets one."""

    def __init__(self, fs=22050, fft_size=1024, hop_size=256, win_length=None, window="hann_window", num_mels=80, fmin=80,
                 fmax=7600, center=True, normalized=False, onesided=True, eps=1e-10, log_base=10.0, device=None,
                 differentiable=False):
        self.differentiable = bool(differentiable)
        self.fft_size = int(fft_size)
        self.hop_size = int(hop_size)
        self.win_length = int(win_length) if win_length is not None else self.fft_size
        self.center, self.normalized, self.onesided = center, normalized, onesided       # stored, ignored (see above)
        self.eps = eps
        self.log_base = log_base
        if log_base not in _LOG_BASES:
            raise ValueError(f"log_base: {log_base} is not supported.")
        if window != "hann_window":
            raise NotImplementedError(f"window {window!r}: only 'hann_window' is implemented on the HIP path")
        n = self.fft_size
        _check_fft_size(n)
        if self.hop_size <= 0 or not 0 < self.win_length <= n:
            raise ValueError(f"need hop_size > 0 and 0 < win_length <= fft_size, got {self.hop_size}, {self.win_length}")
        self.num_mels = int(num_mels)
        if not 0 < self.num_mels <= 256:
            raise NotImplementedError(f"num_mels {num_mels}: the HIP path implements 1 to 256 mel bands")
        fmin = 0 if fmin is None else fmin
        fmax = fs / 2 if fmax is None else fmax
        self.melmat = mel_filterbank(fs, n, self.num_mels, fmin, fmax)          # (n_mels, bins), librosa's layout
        self.window = torch.hann_window(self.win_length)
        self._range, self._weights = sparse_filters(self.melmat)
        self._trange, self._tweights = transposed_filters(self.melmat)
        self._dev = None
        if device is not None:
            self.to(device)

    def to(self, device):
        dev = torch.device(device)
        native.require_gpu(dev)
        if self._dev != dev:
            self._dev = dev
            self._window_d = self.window.to(dev)
            self._range_d = torch.from_numpy(self._range).to(dev)
            self._weights_d = torch.from_numpy(self._weights).to(dev)
            self._trange_d = torch.from_numpy(self._trange).to(dev)
            self._tweights_d = torch.from_numpy(self._tweights).to(dev)
        return self

    def _device_for(self, x):
        if self._dev is None:
            self.to(x.device if x.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
        return self._dev

    def num_frames(self, n_samples):
        return num_frames(n_samples, self.hop_size)

    def check_length(self, n_samples):
        _check_length(n_samples, self.fft_size)

    def _args(self):
        return (self.fft_size, self.hop_size, _ptr(self._window_d), self.win_length, _ptr(self._range_d), _ptr(self._weights_d),
                int(self._weights.size), self.num_mels, _LOG_BASES[self.log_base], float(self.eps))

    def _targs(self):
        return _ptr(self._trange_d), _ptr(self._tweights_d), int(self._tweights.size)

    def forward(self, x):
        """x (B, T) or (B, C, T) -> log-mel (B*C, num_mels, frames) float32 on the device.  Does not synchronise.  With
        ``differentiable=True`` and an ``x`` that requires grad, the result carries the backward (adk_logmel_vjp)."""
        grad = _wants_grad(self.differentiable, x)
        if not grad:
            _no_grad_inputs(x)
        x = _settled(x)
        self.check_length(x.shape[-1])
        dev = self._device_for(x)
        if grad:
            if x.dim() not in (2, 3):
                raise ValueError(f"expected a (B, T) or (B, C, T) waveform, got shape {tuple(x.shape)}")
            return _LogMelFn.apply(x, self)
        return self._logmel(_signals(x, dev))

    def _logmel(self, xs):
        dev = self._dev
        n, T = xs.shape
        out = torch.empty(n, self.num_mels, self.num_frames(T), dtype=torch.float32, device=dev)
        n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps = self._args()
        native.check(native.lib().adk_logmel(_ptr(xs), n, T, n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps, _ptr(out),
                                             native.current_stream(dev)), "adk_logmel")
        return out

    __call__ = forward

    def fold(self, y_hat, y, sum_, count, loss=None):
        """adk_mel_distance: sum_ (float64 [1]) += sum |logmel(y_hat) - logmel(y)|, count (int64 [1]) += elements; loss (float32
        [1] or None) = sum_ / count after the fold.  y_hat, y: contiguous float32 (n, T) on this module's device."""
        dev = self._dev
        n, T = (int(y.shape[0]), int(y.shape[1])) if y is not None else (0, self.fft_size)
        lib = native.lib()
        ws = _workspace(int(lib.adk_mel_workspace_bytes(n, T, self.fft_size, self.hop_size)), "adk_mel_workspace_bytes", dev)
        n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps = self._args()
        native.check(lib.adk_mel_distance(_ptr(y_hat), _ptr(y), n, T, n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps,
                                          _ptr(sum_), _ptr(count), _ptr(ws), _ptr(loss), native.current_stream(dev)),
                     "adk_mel_distance")

    def _vjp(self, xs, g):
        """adk_logmel_vjp: xs (n, T), g (n, num_mels, frames), contiguous float32 on this module's device -> grad (n, T)."""
        dev = self._dev
        n, T = int(xs.shape[0]), int(xs.shape[1])
        if tuple(g.shape) != (n, self.num_mels, self.num_frames(T)) or g.device != xs.device:
            raise ValueError(f"upstream gradient {tuple(g.shape)} on {g.device} does not match the log-mel of {tuple(xs.shape)}")
        grad = torch.empty_like(xs)
        ws = _grad_workspace(n, T, self.fft_size, self.hop_size, dev)
        n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps = self._args()
        native.check(native.lib().adk_logmel_vjp(_ptr(xs), _ptr(g), n, T, n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps,
                                                 *self._targs(), _ptr(ws), _ptr(grad), native.current_stream(dev)),
                     "adk_logmel_vjp")
        return grad

    def _distance_grad(self, a, b, scale, upstream):
        """adk_mel_distance_grad: the gradient with respect to a of scale * upstream[0] * sum |logmel(a) - logmel(b)|."""
        dev = self._dev
        n, T = int(a.shape[0]), int(a.shape[1])
        grad = torch.empty_like(a)
        ws = _grad_workspace(n, T, self.fft_size, self.hop_size, dev)
        n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps = self._args()
        native.check(native.lib().adk_mel_distance_grad(_ptr(a), _ptr(b), n, T, n_fft, hop, win, wl, rng, wts, nw, nm, lb, eps,
                                                        *self._targs(), float(scale), _ptr(upstream), _ptr(ws), _ptr(grad),
                                                        native.current_stream(dev)), "adk_mel_distance_grad")
        return grad


class MultiMelSpectrogramLoss:
    """losses/mel_loss.py:97-156 on the HIP path: mean over resolutions of F.l1_loss(f(y_hat), f(y)).  Same arguments and
    defaults; ``forward(y_hat, y)`` returns a 0-d float32 tensor on the device without synchronising.
    ``differentiable=True`` (not in the reference): a ``y_hat`` that requires grad gets a gradient (adk_mel_distance_grad per
    resolution); ``y`` is the target and may not require grad.  The value is the same either way."""

    def __init__(self, fs=22050, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240],
                 window="hann_window", num_mels=80, fmin=80, fmax=7600, center=True, normalized=False, onesided=True, eps=1e-10,
                 log_base=10.0, device=None, differentiable=False):
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.differentiable = bool(differentiable)
        self.mel_transfers = [MelSpectrogram(fs=fs, fft_size=f, hop_size=h, win_length=w, window=window, num_mels=num_mels,
                                             fmin=fmin, fmax=fmax, center=center, normalized=normalized, onesided=onesided,
                                             eps=eps, log_base=log_base, device=device, differentiable=differentiable)
                              for f, h, w in zip(fft_sizes, hop_sizes, win_lengths)]

    def to(self, device):
        for f in self.mel_transfers:
            f.to(device)
        return self

    @property
    def device(self):
        return self.mel_transfers[0]._dev

    def prepare(self, y_hat, y):
        """Settled, validated, contiguous float32 (n, T) signals on the loss's device."""
        _no_grad_inputs(y) if _wants_grad(self.differentiable, y_hat) else _no_grad_inputs(y_hat, y)
        y_hat, y = _settled(y_hat), _settled(y)
        if tuple(y_hat.shape) != tuple(y.shape):
            raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} must have the same shape")
        for f in self.mel_transfers:
            f.check_length(y.shape[-1])
        dev = self.mel_transfers[0]._device_for(y)
        self.to(dev)
        return _signals(y_hat.detach(), dev), _signals(y, dev)

    def forward(self, y_hat, y):
        a, b = self.prepare(y_hat, y)
        if _wants_grad(self.differentiable, y_hat):
            if a.shape[0] == 0:
                raise ValueError("an empty batch has no gradient")
            return _MelLossFn.apply(lazy_guard.plain(y_hat), self, a, b)
        return self._value(a, b)

    def _value(self, a, b):
        dev = self.device
        R = len(self.mel_transfers)
        sums = torch.zeros(R, dtype=torch.float64, device=dev)
        counts = torch.zeros(R, dtype=torch.int64, device=dev)
        losses = torch.empty(R, dtype=torch.float32, device=dev)
        for r, f in enumerate(self.mel_transfers):
            f.fold(a, b, sums[r:r + 1], counts[r:r + 1], losses[r:r + 1])
        return _mean_f32(losses)

    __call__ = forward


class MelDistance(_Accumulator):
    """The mel-spectrogram loss of a config's ``mel_loss_params``, accumulated on the device over any number of batches.

    ``update(y_hat, y)`` folds the per-resolution L1 sums and element counts without synchronising (lazy-guard results are
    settled first).  ``value()`` is the mean over resolutions of (sum / count) in f64 -- the loss of all folded batches as one
    batch; ``count()`` the elements folded per resolution; ``reset()`` zeroes the totals.  ``value()`` and ``count()``
    synchronise."""

    def __init__(self, loss_params, device):
        self.loss = MultiMelSpectrogramLoss(**dict(loss_params), device=device)
        self.device = self.loss.device
        self._init_totals(len(self.loss.mel_transfers), self.device)

    def update(self, y_hat, y):
        a, b = self.loss.prepare(y_hat, y)
        if a.shape[0] == 0:
            return self
        for r, f in enumerate(self.loss.mel_transfers):
            f.fold(a, b, self._sum[r:r + 1], self._count[r:r + 1])
        return self


def from_config(config, device=None, differentiable=False):
    """The loss a training config enables (codecTrain.py:202-205): MultiMelSpectrogramLoss(**config['mel_loss_params']) when
    ``use_mel_loss`` is true, else None."""
    if not config.get("use_mel_loss", False):
        return None
    return MultiMelSpectrogramLoss(**config["mel_loss_params"], device=device, differentiable=differentiable)
