"""Waveform-shape loss on the device (adk_shape_distance) and its backward (adk_grad_shape_distance).

Mirrors ``losses/waveform_loss.py``: ``WaveformShapeLoss`` (lines 15-38) is ``L1Loss(MaxPool1d(winlen)(|y_hat|),
MaxPool1d(winlen)(|y|))`` -- the pooling stride is ``winlen``, so a signal of T samples gives ``T // winlen`` windows and the
tail is dropped -- and ``MultiWindowShapeLoss`` (41-75) its mean over window lengths.  The reference's trainers build it from
``config['shape_loss_params']`` as the third term of the metric loss (trainer/trainerGAN.py:214-241).

Forward only by default: an input that requires grad while grad is enabled raises NotImplementedError.  Built with
``differentiable=True``, ``WaveformShapeLoss`` and ``MultiWindowShapeLoss`` give the generated signal ``y_hat`` -- never the target
``y`` -- a gradient through ``torch.autograd``: per window, sign(max|y_hat| - max|y|) sign(y_hat[i]) / (R windows) at the first
index i of the window's max |y_hat| (what MaxPool1d's backward selects) and 0 elsewhere, the dropped tail included.  Windows are
disjoint, so the gradient is bitwise reproducible.  The backward is once-differentiable.  ``ShapeDistance`` stays forward only.
"""
import torch

from . import lazy_guard, native
from .loss_common import (_Accumulator, _device_of, _mean_f32, _no_grad_inputs, _ptr, _settled, _signals, _wants_grad,
                          _workspace)


def num_windows(n_samples, winlen):
    """Windows of MaxPool1d(winlen): T // winlen."""
    return int(n_samples) // int(winlen)


def _prepare(y_hat, y, winlens, differentiable=False):
    """Settled, validated, contiguous float32 (n, T) signals on a HIP device."""
    _no_grad_inputs(y) if _wants_grad(differentiable, y_hat) else _no_grad_inputs(y_hat, y)
    y_hat, y = _settled(y_hat), _settled(y)
    if tuple(y_hat.shape) != tuple(y.shape):
        raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} must have the same shape")
    for w in winlens:
        if y.shape[-1] < w:
            raise ValueError(f"input length {y.shape[-1]} is shorter than winlen {w} (MaxPool1d raises for it too)")
    dev = _device_of(y)
    return _signals(y_hat.detach(), dev), _signals(y, dev)


def _loss_value(losses, a, b):
    """The mean over the window lengths `losses` as a 0-d float32 device tensor."""
    R = len(losses)
    sums = torch.zeros(R, dtype=torch.float64, device=b.device)
    counts = torch.zeros(R, dtype=torch.int64, device=b.device)
    res = torch.empty(R, dtype=torch.float32, device=b.device)
    for r, f in enumerate(losses):
        f.fold(a, b, sums[r:r + 1], counts[r:r + 1], res[r:r + 1])
    return _mean_f32(res)


class _ShapeLossFn(torch.autograd.Function):
    """The mean over a list of WaveformShapeLoss window lengths with a backward with respect to y_hat: the fold path's value, and
    per window length adk_grad_shape_distance, scaled by 1 / (R windows) and summed over the window lengths in their order."""

    @staticmethod
    def forward(ctx, y_hat, losses, a, b):
        ctx.losses, ctx.like = losses, (y_hat.shape, y_hat.device, y_hat.dtype)
        ctx.save_for_backward(a, b)
        return _loss_value(losses, a, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (a, b), losses, (shape, device, dtype) = ctx.saved_tensors, ctx.losses, ctx.like
        up = g.to(device=a.device, dtype=torch.float32).reshape(1).contiguous()
        R = len(losses)
        if R == 1:
            grad = losses[0]._distance_grad(a, b, 1.0 / float(a.shape[0] * num_windows(a.shape[1], losses[0].winlen)), up)
            return grad.reshape(shape).to(device=device, dtype=dtype), None, None, None
        # Several window lengths may choose one sample with opposite signs, and what is left can be a small part of the largest
        # term (1/150 - 1/228 - 1/462 = 1/57 of 1/150): the kernel writes the exact +-upstream, the scales are applied and the
        # window lengths added in f64, and the sum is rounded to f32 once.
        grad = None
        for f in losses:
            windows = a.shape[0] * num_windows(a.shape[1], f.winlen)
            gr = f._distance_grad(a, b, 1.0, up).to(torch.float64) * (1.0 / (float(windows) * R))
            grad = gr if grad is None else grad + gr
        return grad.to(torch.float32).reshape(shape).to(device=device, dtype=dtype), None, None, None


def _forward(losses, y_hat, y, differentiable):
    a, b = _prepare(y_hat, y, [f.winlen for f in losses], differentiable)
    if _wants_grad(differentiable, y_hat):
        if a.shape[0] == 0:
            raise ValueError("an empty batch has no gradient")
        return _ShapeLossFn.apply(lazy_guard.plain(y_hat), losses, a, b)
    return _loss_value(losses, a, b)


class WaveformShapeLoss:
    """losses/waveform_loss.py:15-38 on the HIP path; ``forward(y_hat, y)`` returns a 0-d float32 tensor on the device
    without synchronising.  ``differentiable=True`` (not in the reference, whose modules always are): a ``y_hat`` that requires
    grad gets a gradient (adk_grad_shape_distance); ``y`` is the target and may not require grad.  The value is the same either
    way."""

    def __init__(self, winlen, differentiable=False):
        self.differentiable = bool(differentiable)
        self.winlen = int(winlen)
        if self.winlen <= 0:
            raise ValueError(f"need winlen > 0, got {winlen}")

    def fold(self, y_hat, y, sum_, count, loss=None):
        """adk_shape_distance: sum_ (float64 [1]) += sum |max|y_hat| - max|y||, count (int64 [1]) += windows; loss (float32 [1]
        or None) = sum_ / count after the fold.  y_hat, y: contiguous float32 (n, T) on one HIP device."""
        dev = y.device
        n, T = int(y.shape[0]), int(y.shape[1])
        lib = native.lib()
        ws = _workspace(int(lib.adk_shape_workspace_bytes(n, T, self.winlen)), "adk_shape_workspace_bytes", dev)
        native.check(lib.adk_shape_distance(_ptr(y_hat), _ptr(y), n, T, self.winlen, _ptr(sum_), _ptr(count), _ptr(ws), _ptr(loss),
                                            native.current_stream(dev)), "adk_shape_distance")

    def _distance_grad(self, y_hat, y, scale, upstream):
        """adk_grad_shape_distance: the gradient with respect to y_hat of scale * upstream[0] * sum |max|y_hat| - max|y||."""
        dev = y.device
        n, T = int(y.shape[0]), int(y.shape[1])
        grad = torch.empty_like(y_hat)
        native.check(native.lib().adk_grad_shape_distance(_ptr(y_hat), _ptr(y), n, T, self.winlen, float(scale), _ptr(upstream),
                                                          _ptr(grad), native.current_stream(dev)), "adk_grad_shape_distance")
        return grad

    def forward(self, y_hat, y):
        return _forward([self], y_hat, y, self.differentiable)

    __call__ = forward


class MultiWindowShapeLoss:
    """losses/waveform_loss.py:41-75 on the HIP path: the mean over window lengths.  Same argument and default.
    ``differentiable=True`` (not in the reference): a ``y_hat`` that requires grad gets a gradient, the window lengths' gradients
    added in their order; ``y`` may not require grad."""

    def __init__(self, winlen=[300, 200, 100], differentiable=False):
        self.differentiable = bool(differentiable)
        self.shape_losses = [WaveformShapeLoss(wl, differentiable=differentiable) for wl in winlen]

    def prepare(self, y_hat, y):
        return _prepare(y_hat, y, [f.winlen for f in self.shape_losses], self.differentiable)

    def forward(self, y_hat, y):
        return _forward(self.shape_losses, y_hat, y, self.differentiable)

    __call__ = forward


class ShapeDistance(_Accumulator):
    """The shape loss of a config's ``shape_loss_params``, accumulated on the device over any number of batches.

    ``update(y_hat, y)`` folds the per-window-length sums and window counts without synchronising.  ``value()`` is the mean over
    window lengths of (sum / count) in f64 -- the loss of all folded batches as one batch; ``count()`` the windows folded per
    window length; ``reset()`` zeroes the totals.  ``value()`` and ``count()`` synchronise."""

    def __init__(self, loss_params, device):
        self.loss = MultiWindowShapeLoss(**dict(loss_params))
        self.device = native.require_gpu(torch.device(device))
        self._init_totals(len(self.loss.shape_losses), self.device)

    def update(self, y_hat, y):
        a, b = self.loss.prepare(y_hat, y)
        a, b = a.to(self.device), b.to(self.device)
        if a.shape[0] == 0:
            return self
        for r, f in enumerate(self.loss.shape_losses):
            f.fold(a, b, self._sum[r:r + 1], self._count[r:r + 1])
        return self


def from_config(config, device=None, differentiable=False):
    """The loss a training config enables: MultiWindowShapeLoss(**config['shape_loss_params']) when ``use_shape_loss`` is
    true, else None.  ``device`` is accepted for symmetry with the other losses; the loss runs where its inputs are."""
    if not config.get("use_shape_loss", False):
        return None
    return MultiWindowShapeLoss(**config["shape_loss_params"], differentiable=differentiable)
