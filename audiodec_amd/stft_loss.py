"""Multi-resolution STFT loss on the device (adk_stft_mag, adk_stft_distance, adk_mag_distance) and its backward
(adk_grad_stft_mag, adk_grad_stft_distance).

Mirrors ``losses/stft_loss.py``: ``stft`` (lines 19-35), ``SpectralConvergenceLoss``, ``LogSTFTMagnitudeLoss``, ``STFTLoss``
(38-117) and ``MultiResolutionSTFTLoss`` (120-170), which the reference's trainers build from ``config['stft_loss_params']``
and use as the second term of the metric loss (trainer/trainerGAN.py:214-241).  x is the predicted signal, y the ground truth:

    sc  = || y_mag - x_mag ||_F / || y_mag ||_F        mag = mean | log y_mag - log x_mag |

Each resolution runs one HIP kernel that frames both signals with reflect padding, transforms them and folds the three sums the
two terms need into an f64 accumulator on the device, without ever writing a magnitude.  The window is
``getattr(torch, window)(win_length)``: any torch window function, the kernel takes its values.

Forward only by default: an input that requires grad while grad is enabled raises NotImplementedError.  Built (``stft``: called)
with ``differentiable=True``, ``stft``, ``STFTLoss`` and ``MultiResolutionSTFTLoss`` give the predicted signal ``x`` -- never the
target ``y`` -- a gradient through ``torch.autograd``: each frame's forward is recomputed and walked back on the device, the two
terms' upstream gradients and the forward's folded sums are read there (no host synchronisation), and the frame gradients are
overlap-added in a fixed order, so the gradient is bitwise reproducible like the value.  The backward is once-differentiable.
``SpectralConvergenceLoss`` / ``LogSTFTMagnitudeLoss`` on given magnitude tensors and ``STFTDistance`` stay forward only.
"""
import numpy as np
import torch

from . import lazy_guard, native
from .loss_common import (_check_fft_size, _check_length, _device_of, _mean_f32, _no_grad_inputs, _ptr, _settled, _signals,
                          _wants_grad, _workspace, num_frames)


def _grad_workspace(n, T, n_fft, hop, dev):
    ws_bytes = int(native.lib().adk_grad_stft_workspace_bytes(n, T, n_fft, hop))
    if ws_bytes < 0:
        native.check(ws_bytes, "adk_grad_stft_workspace_bytes")
    return torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)


def _stft_mag(xs, fft_size, hop_size, win, win_length, eps):
    n, T = xs.shape
    out = torch.empty(n, num_frames(T, hop_size), fft_size // 2 + 1, dtype=torch.float32, device=xs.device)
    native.check(native.lib().adk_stft_mag(_ptr(xs), n, T, fft_size, hop_size, _ptr(win), win_length, float(eps), _ptr(out),
                                           native.current_stream(xs.device)), "adk_stft_mag")
    return out


class _StftMagFn(torch.autograd.Function):
    """stft() with a backward: adk_stft_mag, and adk_grad_stft_mag on the saved signal."""

    @staticmethod
    def forward(ctx, x, xs, win, args):
        ctx.args, ctx.like = args, (x.shape, x.device, x.dtype)
        ctx.save_for_backward(xs, win)
        return _stft_mag(xs, args[0], args[1], win, args[2], args[3])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (xs, win), (fft_size, hop_size, win_length, eps), (shape, device, dtype) = ctx.saved_tensors, ctx.args, ctx.like
        dev = xs.device
        n, T = int(xs.shape[0]), int(xs.shape[1])
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(xs)
        ws = _grad_workspace(n, T, fft_size, hop_size, dev)
        native.check(native.lib().adk_grad_stft_mag(_ptr(xs), _ptr(g), n, T, fft_size, hop_size, _ptr(win), win_length, float(eps),
                                                   _ptr(ws), _ptr(grad), native.current_stream(dev)), "adk_grad_stft_mag")
        return grad.reshape(shape).to(device=device, dtype=dtype), None, None, None


class _StftLossFn(torch.autograd.Function):
    """(sc, mag) of a list of STFTLoss resolutions with a backward with respect to x: the fold path's values, the forward's (R, 3)
    f64 sums kept on the device, and per resolution adk_grad_stft_distance with scale_sc = 1 / R and scale_mag = 1 / (R count),
    summed over the resolutions in their order."""

    @staticmethod
    def forward(ctx, x, losses, a, b):
        ctx.losses, ctx.like = losses, (x.shape, x.device, x.dtype)
        sc, mag, sums = _loss_value(losses, a, b)
        ctx.save_for_backward(a, b, sums)
        return sc, mag

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sc, g_mag):
        (a, b, sums), losses, (shape, device, dtype) = ctx.saved_tensors, ctx.losses, ctx.like
        up = torch.stack([g_sc.reshape(()), g_mag.reshape(())]).to(device=a.device, dtype=torch.float32).contiguous()
        R = len(losses)
        grad = None
        for r, f in enumerate(losses):
            count = a.shape[0] * f.num_frames(a.shape[1]) * (f.fft_size // 2 + 1)
            gr = f._distance_grad(a, b, sums[r], 1.0 / R, up[0:1], 1.0 / (float(count) * R), up[1:2])
            grad = gr if grad is None else grad + gr
        return grad.reshape(shape).to(device=device, dtype=dtype), None, None, None


def _loss_value(losses, a, b):
    """(sc, mag, sums): the means over the resolutions `losses` of the two terms as 0-d float32 device tensors, and the (R, 3)
    float64 sums the folds left on the device."""
    dev = a.device
    R = len(losses)
    sums = torch.zeros(R, 3, dtype=torch.float64, device=dev)
    counts = torch.zeros(R, dtype=torch.int64, device=dev)
    res = torch.empty(R, 2, dtype=torch.float32, device=dev)
    for r, f in enumerate(losses):
        f.fold(a, b, sums[r], counts[r:r + 1], res[r, 0:1], res[r, 1:2])
    return _mean_f32(res[:, 0]), _mean_f32(res[:, 1]), sums


def _prepare(losses, x, y, differentiable):
    """Settled, validated, contiguous float32 (n, T) signals on the device of the resolutions `losses`."""
    _no_grad_inputs(y) if _wants_grad(differentiable, x) else _no_grad_inputs(x, y)
    x, y = _settled(x), _settled(y)
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have the same shape")
    for f in losses:
        f.check_length(y.shape[-1])
    dev = losses[0]._device_for(y)
    for f in losses:
        f.to(dev)
    return _signals(x.detach(), dev), _signals(y, dev)


def _forward(losses, x, y, differentiable):
    a, b = _prepare(losses, x, y, differentiable)
    if _wants_grad(differentiable, x):
        if a.shape[0] == 0:
            raise ValueError("an empty batch has no gradient")
        return _StftLossFn.apply(lazy_guard.plain(x), losses, a, b)
    return _loss_value(losses, a, b)[:2]


def stft(x, fft_size, hop_size, win_length, window, eps=1e-7, differentiable=False):
    """losses/stft_loss.py:19-35: x (B, T), window a (win_length,) tensor -> magnitudes (B, frames, fft_size // 2 + 1) float32
    on the device.  Does not synchronise.  ``differentiable=True`` (not in the reference, whose function always is): an ``x`` that
    requires grad gets one (adk_grad_stft_mag)."""
    fft_size, hop_size, win_length = int(fft_size), int(hop_size), int(win_length)
    _check_fft_size(fft_size)
    grad = _wants_grad(differentiable, x)
    if not grad:
        _no_grad_inputs(x)
    x = _settled(x)
    if x.dim() != 2:
        raise ValueError(f"expected a (B, T) waveform, got shape {tuple(x.shape)}")
    if hop_size <= 0 or not 0 < win_length <= fft_size or tuple(window.shape) != (win_length,):
        raise ValueError(f"need hop_size > 0, 0 < win_length <= fft_size and a window of win_length values, got {hop_size}, "
                         f"{win_length}, {tuple(window.shape)}")
    _check_length(x.shape[-1], fft_size)
    dev = _device_of(x)
    xs = _signals(x.detach(), dev)
    win = window.detach().to(device=dev, dtype=torch.float32).contiguous()
    if grad:
        if xs.shape[0] == 0:
            raise ValueError("an empty batch has no gradient")
        return _StftMagFn.apply(x, xs, win, (fft_size, hop_size, win_length, float(eps)))
    return _stft_mag(xs, fft_size, hop_size, win, win_length, eps)


def _mag_distance(x_mag, y_mag):
    """(sc, mag) of two magnitude tensors as 0-d float32 device tensors (adk_mag_distance)."""
    _no_grad_inputs(x_mag, y_mag)
    x_mag, y_mag = _settled(x_mag), _settled(y_mag)
    if tuple(x_mag.shape) != tuple(y_mag.shape):
        raise ValueError(f"x_mag {tuple(x_mag.shape)} and y_mag {tuple(y_mag.shape)} must have the same shape")
    dev = _device_of(y_mag)
    a = x_mag.to(device=dev, dtype=torch.float32).contiguous()
    b = y_mag.to(device=dev, dtype=torch.float32).contiguous()
    n = a.numel()
    lib = native.lib()
    ws = _workspace(int(lib.adk_mag_distance_workspace_bytes(n)), "adk_mag_distance_workspace_bytes", dev)
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    res = torch.empty(2, dtype=torch.float32, device=dev)
    native.check(lib.adk_mag_distance(_ptr(a), _ptr(b), n, _ptr(sums), _ptr(count), _ptr(ws), _ptr(res[0:1]), _ptr(res[1:2]),
                                      native.current_stream(dev)), "adk_mag_distance")
    return res[0], res[1]


class SpectralConvergenceLoss:
    """losses/stft_loss.py:38-56: ||y_mag - x_mag||_F / ||y_mag||_F of two magnitude tensors."""

    def forward(self, x_mag, y_mag):
        return _mag_distance(x_mag, y_mag)[0]

    __call__ = forward


class LogSTFTMagnitudeLoss:
    """losses/stft_loss.py:59-77: F.l1_loss(log y_mag, log x_mag) of two magnitude tensors."""

    def forward(self, x_mag, y_mag):
        return _mag_distance(x_mag, y_mag)[1]

    __call__ = forward


class STFTLoss:
    """losses/stft_loss.py:80-117 on the HIP path.  Same arguments and defaults; ``forward(x, y)`` returns ``(sc, mag)``.
    ``differentiable=True`` (not in the reference, whose modules always are): an ``x`` that requires grad gets a gradient from
    both terms (adk_grad_stft_distance); ``y`` is the target and may not require grad.  The values are the same either way."""

    def __init__(self, fft_size=1024, hop_size=120, win_length=600, window="hann_window", device=None, differentiable=False):
        self.differentiable = bool(differentiable)
        self.fft_size, self.hop_size, self.win_length = int(fft_size), int(hop_size), int(win_length)
        _check_fft_size(self.fft_size)
        if self.hop_size <= 0 or not 0 < self.win_length <= self.fft_size:
            raise ValueError(f"need hop_size > 0 and 0 < win_length <= fft_size, got {self.hop_size}, {self.win_length}")
        self.eps = 1e-7                                                         # stft()'s default, which STFTLoss never overrides
        self.spectral_convergence_loss = SpectralConvergenceLoss()
        self.log_stft_magnitude_loss = LogSTFTMagnitudeLoss()
        self.window = getattr(torch, window)(self.win_length).to(torch.float32)
        self._dev = None
        if device is not None:
            self.to(device)

    def to(self, device):
        dev = native.require_gpu(torch.device(device))
        if self._dev != dev:
            self._dev = dev
            self._window_d = self.window.to(dev)
        return self

    def _device_for(self, x):
        if self._dev is None:
            self.to(x.device if x.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
        return self._dev

    def num_frames(self, n_samples):
        return num_frames(n_samples, self.hop_size)

    def check_length(self, n_samples):
        _check_length(n_samples, self.fft_size)

    def fold(self, x, y, sums, count, sc=None, mag=None):
        """adk_stft_distance: sums (float64 [3]) += (sum d^2, sum y_mag^2, sum |dlog|), count (int64 [1]) += elements; sc, mag
        (float32 [1] or None) from the totals after the fold.  x, y: contiguous float32 (n, T) on this module's device."""
        dev = self._dev
        n, T = int(y.shape[0]), int(y.shape[1])
        lib = native.lib()
        ws = _workspace(int(lib.adk_stft_workspace_bytes(n, T, self.fft_size, self.hop_size)), "adk_stft_workspace_bytes", dev)
        native.check(lib.adk_stft_distance(_ptr(x), _ptr(y), n, T, self.fft_size, self.hop_size, _ptr(self._window_d),
                                           self.win_length, float(self.eps), _ptr(sums), _ptr(count), _ptr(ws), _ptr(sc), _ptr(mag),
                                           native.current_stream(dev)), "adk_stft_distance")

    def _distance_grad(self, x, y, sums, scale_sc, up_sc, scale_mag, up_mag):
        """adk_grad_stft_distance: the gradient with respect to x of scale_sc up_sc[0] sc + scale_mag up_mag[0] sum |dlog|, sums
        (float64 [3]) being what fold(x, y, ...) left on the device; up_sc, up_mag float32 [1] on the device."""
        dev = self._dev
        n, T = int(x.shape[0]), int(x.shape[1])
        grad = torch.empty_like(x)
        ws = _grad_workspace(n, T, self.fft_size, self.hop_size, dev)
        native.check(native.lib().adk_grad_stft_distance(_ptr(x), _ptr(y), n, T, self.fft_size, self.hop_size, _ptr(self._window_d),
                                                         self.win_length, float(self.eps), _ptr(sums), float(scale_sc), _ptr(up_sc),
                                                         float(scale_mag), _ptr(up_mag), _ptr(ws), _ptr(grad),
                                                         native.current_stream(dev)), "adk_grad_stft_distance")
        return grad

    def forward(self, x, y):
        return _forward([self], x, y, self.differentiable)

    __call__ = forward


class MultiResolutionSTFTLoss:
    """losses/stft_loss.py:120-170 on the HIP path: the means over resolutions of the two terms.  Same arguments and defaults;
    ``forward(x, y)`` returns ``(sc_loss, mag_loss)`` as 0-d float32 tensors on the device without synchronising.
    ``differentiable=True`` (not in the reference): an ``x`` that requires grad gets a gradient from both terms, the
    resolutions' gradients added in their order; ``y`` may not require grad.  The values are the same either way."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
                 device=None, differentiable=False):
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.differentiable = bool(differentiable)
        self.stft_losses = [STFTLoss(f, h, w, window, device=device, differentiable=differentiable)
                            for f, h, w in zip(fft_sizes, hop_sizes, win_lengths)]

    def to(self, device):
        for f in self.stft_losses:
            f.to(device)
        return self

    @property
    def device(self):
        return self.stft_losses[0]._dev

    def prepare(self, x, y):
        """Settled, validated, contiguous float32 (n, T) signals on the loss's device."""
        return _prepare(self.stft_losses, x, y, self.differentiable)

    def forward(self, x, y):
        return _forward(self.stft_losses, x, y, self.differentiable)

    __call__ = forward


class STFTDistance:
    """The STFT loss of a config's ``stft_loss_params``, accumulated on the device over any number of batches.

    ``update(y_hat, y)`` folds the per-resolution sums and element counts without synchronising (lazy-guard results are settled
    first).  ``value()`` is ``(sc, mag)`` of all folded batches as one batch, in f64: the means over resolutions of
    sqrt(sum d^2) / sqrt(sum y^2) and of sum |dlog| / count; ``count()`` the elements folded per resolution; ``reset()``
    zeroes the totals.  ``value()`` and ``count()`` synchronise."""

    def __init__(self, loss_params, device):
        self.loss = MultiResolutionSTFTLoss(**dict(loss_params), device=device)
        self.device = self.loss.device
        R = len(self.loss.stft_losses)
        self._sums = torch.zeros(R, 3, dtype=torch.float64, device=self.device)
        self._count = torch.zeros(R, dtype=torch.int64, device=self.device)

    def reset(self):
        self._sums.zero_()
        self._count.zero_()
        return self

    def update(self, y_hat, y):
        a, b = self.loss.prepare(y_hat, y)
        if a.shape[0] == 0:
            return self
        for r, f in enumerate(self.loss.stft_losses):
            f.fold(a, b, self._sums[r], self._count[r:r + 1])
        return self

    def count(self):
        return [int(c) for c in self._count.cpu()]

    def value(self):
        s, c = self._sums.cpu().numpy(), self._count.cpu().numpy()
        if (c == 0).any():
            return float("nan"), float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.mean(np.sqrt(s[:, 0]) / np.sqrt(s[:, 1]))), float(np.mean(s[:, 2] / c))


def from_config(config, device=None, differentiable=False):
    """The loss a training config enables: MultiResolutionSTFTLoss(**config['stft_loss_params']) when ``use_stft_loss`` is
    true, else None."""
    if not config.get("use_stft_loss", False):
        return None
    return MultiResolutionSTFTLoss(**config["stft_loss_params"], device=device, differentiable=differentiable)
