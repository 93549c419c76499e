"""Multi-resolution STFT loss on the device (adk_stft_mag, adk_stft_distance, adk_mag_distance).

Mirrors ``losses/stft_loss.py``: ``stft`` (lines 19-35), ``SpectralConvergenceLoss``, ``LogSTFTMagnitudeLoss``, ``STFTLoss``
(38-117) and ``MultiResolutionSTFTLoss`` (120-170), which the reference's trainers build from ``config['stft_loss_params']``
and use as the second term of the metric loss (trainer/trainerGAN.py:214-241).  x is the predicted signal, y the ground truth:

    sc  = || y_mag - x_mag ||_F / || y_mag ||_F        mag = mean | log y_mag - log x_mag |

Each resolution runs one HIP kernel that frames both signals with reflect padding, transforms them and folds the three sums the
two terms need into an f64 accumulator on the device, without ever writing a magnitude.  The window is
``getattr(torch, window)(win_length)``: any torch window function, the kernel takes its values.

Forward only: an input that requires grad while grad is enabled raises NotImplementedError.
"""
import numpy as np
import torch

from . import native
from .loss_common import (_check_fft_size, _check_length, _device_of, _mean_f32, _no_grad_inputs, _ptr, _settled, _signals,
                          _workspace, num_frames)


def stft(x, fft_size, hop_size, win_length, window, eps=1e-7):
    """losses/stft_loss.py:19-35: x (B, T), window a (win_length,) tensor -> magnitudes (B, frames, fft_size // 2 + 1) float32
    on the device.  Does not synchronise."""
    fft_size, hop_size, win_length = int(fft_size), int(hop_size), int(win_length)
    _check_fft_size(fft_size)
    _no_grad_inputs(x)
    x = _settled(x)
    if x.dim() != 2:
        raise ValueError(f"expected a (B, T) waveform, got shape {tuple(x.shape)}")
    if hop_size <= 0 or not 0 < win_length <= fft_size or tuple(window.shape) != (win_length,):
        raise ValueError(f"need hop_size > 0, 0 < win_length <= fft_size and a window of win_length values, got {hop_size}, "
                         f"{win_length}, {tuple(window.shape)}")
    _check_length(x.shape[-1], fft_size)
    dev = _device_of(x)
    xs = _signals(x, dev)
    win = window.to(device=dev, dtype=torch.float32).contiguous()
    n, T = xs.shape
    out = torch.empty(n, num_frames(T, hop_size), fft_size // 2 + 1, dtype=torch.float32, device=dev)
    native.check(native.lib().adk_stft_mag(_ptr(xs), n, T, fft_size, hop_size, _ptr(win), win_length, float(eps), _ptr(out),
                                           native.current_stream(dev)), "adk_stft_mag")
    return out


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
    """losses/stft_loss.py:80-117 on the HIP path.  Same arguments and defaults; ``forward(x, y)`` returns ``(sc, mag)``."""

    def __init__(self, fft_size=1024, hop_size=120, win_length=600, window="hann_window", device=None):
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

    def forward(self, x, y):
        _no_grad_inputs(x, y)
        x, y = _settled(x), _settled(y)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have the same shape")
        self.check_length(y.shape[-1])
        dev = self._device_for(y)
        a, b = _signals(x, dev), _signals(y, dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        res = torch.empty(2, dtype=torch.float32, device=dev)
        self.fold(a, b, sums, count, res[0:1], res[1:2])
        return res[0], res[1]

    __call__ = forward


class MultiResolutionSTFTLoss:
    """losses/stft_loss.py:120-170 on the HIP path: the means over resolutions of the two terms.  Same arguments and defaults;
    ``forward(x, y)`` returns ``(sc_loss, mag_loss)`` as 0-d float32 tensors on the device without synchronising."""

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
                 device=None):
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.stft_losses = [STFTLoss(f, h, w, window, device=device) for f, h, w in zip(fft_sizes, hop_sizes, win_lengths)]

    def to(self, device):
        for f in self.stft_losses:
            f.to(device)
        return self

    @property
    def device(self):
        return self.stft_losses[0]._dev

    def prepare(self, x, y):
        """Settled, validated, contiguous float32 (n, T) signals on the loss's device."""
        _no_grad_inputs(x, y)
        x, y = _settled(x), _settled(y)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have the same shape")
        for f in self.stft_losses:
            f.check_length(y.shape[-1])
        dev = self.stft_losses[0]._device_for(y)
        self.to(dev)
        return _signals(x, dev), _signals(y, dev)

    def forward(self, x, y):
        a, b = self.prepare(x, y)
        dev = self.device
        R = len(self.stft_losses)
        sums = torch.zeros(R, 3, dtype=torch.float64, device=dev)
        counts = torch.zeros(R, dtype=torch.int64, device=dev)
        res = torch.empty(R, 2, dtype=torch.float32, device=dev)
        for r, f in enumerate(self.stft_losses):
            f.fold(a, b, sums[r], counts[r:r + 1], res[r, 0:1], res[r, 1:2])
        return _mean_f32(res[:, 0]), _mean_f32(res[:, 1])

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


def from_config(config, device=None):
    """The loss a training config enables: MultiResolutionSTFTLoss(**config['stft_loss_params']) when ``use_stft_loss`` is
    true, else None."""
    if not config.get("use_stft_loss", False):
        return None
    return MultiResolutionSTFTLoss(**config["stft_loss_params"], device=device)
