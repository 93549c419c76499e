"""Waveform-shape loss on the device (adk_shape_distance).

Mirrors ``losses/waveform_loss.py``: ``WaveformShapeLoss`` (lines 15-38) is ``L1Loss(MaxPool1d(winlen)(|y_hat|),
MaxPool1d(winlen)(|y|))`` -- the pooling stride is ``winlen``, so a signal of T samples gives ``T // winlen`` windows and the
tail is dropped -- and ``MultiWindowShapeLoss`` (41-75) its mean over window lengths.  The reference's trainers build it from
``config['shape_loss_params']`` as the third term of the metric loss (trainer/trainerGAN.py:214-241).

Forward only: an input that requires grad while grad is enabled raises NotImplementedError.
"""
import torch

from . import native
from .loss_common import _Accumulator, _device_of, _mean_f32, _no_grad_inputs, _ptr, _settled, _signals, _workspace


def num_windows(n_samples, winlen):
    """Windows of MaxPool1d(winlen): T // winlen."""
    return int(n_samples) // int(winlen)


def _prepare(y_hat, y, winlens):
    """Settled, validated, contiguous float32 (n, T) signals on a HIP device."""
    _no_grad_inputs(y_hat, y)
    y_hat, y = _settled(y_hat), _settled(y)
    if tuple(y_hat.shape) != tuple(y.shape):
        raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} must have the same shape")
    for w in winlens:
        if y.shape[-1] < w:
            raise ValueError(f"input length {y.shape[-1]} is shorter than winlen {w} (MaxPool1d raises for it too)")
    dev = _device_of(y)
    return _signals(y_hat, dev), _signals(y, dev)


class WaveformShapeLoss:
    """losses/waveform_loss.py:15-38 on the HIP path; ``forward(y_hat, y)`` returns a 0-d float32 tensor on the device
    without synchronising."""

    def __init__(self, winlen):
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

    def forward(self, y_hat, y):
        a, b = _prepare(y_hat, y, [self.winlen])
        sum_ = torch.zeros(1, dtype=torch.float64, device=b.device)
        count = torch.zeros(1, dtype=torch.int64, device=b.device)
        loss = torch.empty(1, dtype=torch.float32, device=b.device)
        self.fold(a, b, sum_, count, loss)
        return loss[0]

    __call__ = forward


class MultiWindowShapeLoss:
    """losses/waveform_loss.py:41-75 on the HIP path: the mean over window lengths.  Same argument and default."""

    def __init__(self, winlen=[300, 200, 100]):
        self.shape_losses = [WaveformShapeLoss(wl) for wl in winlen]

    def prepare(self, y_hat, y):
        return _prepare(y_hat, y, [f.winlen for f in self.shape_losses])

    def forward(self, y_hat, y):
        a, b = self.prepare(y_hat, y)
        R = len(self.shape_losses)
        sums = torch.zeros(R, dtype=torch.float64, device=b.device)
        counts = torch.zeros(R, dtype=torch.int64, device=b.device)
        losses = torch.empty(R, dtype=torch.float32, device=b.device)
        for r, f in enumerate(self.shape_losses):
            f.fold(a, b, sums[r:r + 1], counts[r:r + 1], losses[r:r + 1])
        return _mean_f32(losses)

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


def from_config(config, device=None):
    """The loss a training config enables: MultiWindowShapeLoss(**config['shape_loss_params']) when ``use_shape_loss`` is
    true, else None.  ``device`` is accepted for symmetry with the other losses; the loss runs where its inputs are."""
    if not config.get("use_shape_loss", False):
        return None
    return MultiWindowShapeLoss(**config["shape_loss_params"])
