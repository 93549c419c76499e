"""What the device metric losses share (mel.py, stft_loss.py, waveform_loss.py): input handling, the STFT shape checks, the
f64 slab workspace, the f32 mean over resolutions and the per-resolution accumulator."""
import ctypes as C

import numpy as np
import torch

from . import native
from .lazy_guard import settled as _settled


def num_frames(n_samples, hop_size):
    """Frames of torch.stft(center=True): 1 + T // hop."""
    return 1 + int(n_samples) // int(hop_size)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _no_grad_inputs(*ts):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts):
        raise NotImplementedError("the HIP metric losses (mel, STFT, shape) are forward only: run them under torch.no_grad() or "
                                  "detach the inputs")


def _wants_grad(differentiable, x):
    return bool(differentiable) and torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad


def _signals(x, device):
    """(B, T) or (B, C, T) -> contiguous float32 (B*C, T) on `device` (MelSpectrogram.forward's reshape)."""
    if x.dim() == 3:
        x = x.reshape(-1, x.size(2))
    if x.dim() != 2:
        raise ValueError(f"expected a (B, T) or (B, C, T) waveform, got shape {tuple(x.shape)}")
    return x.to(device=device, dtype=torch.float32).contiguous()


def _check_fft_size(n):
    if n < 256 or n > 4096 or n & (n - 1):
        raise NotImplementedError(f"fft_size {n}: the HIP path implements powers of two from 256 to 4096")


def _check_length(n_samples, fft_size):
    if n_samples <= fft_size // 2:
        raise ValueError(f"input length {n_samples}: reflect padding of fft_size // 2 = {fft_size // 2} needs more than "
                         f"{fft_size // 2} samples (torch.stft raises for it too)")


def _workspace(n_bytes, what, dev):
    """The f64 slab an adk_*_workspace_bytes call asked for (None for 0 bytes; a negative count is that call's error)."""
    if n_bytes < 0:
        native.check(n_bytes, what)
    return torch.empty((n_bytes + 7) // 8, dtype=torch.float64, device=dev) if n_bytes else None


def _device_of(x):
    dev = x.device if x.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    return native.require_gpu(dev)


def _mean_f32(terms):
    """terms[0] + terms[1] + ... then / R, in f32 as the reference adds its per-resolution losses; one term is returned as is."""
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    return total if len(terms) == 1 else total / len(terms)


class _Accumulator:
    """A per-resolution f64 sum and element count on the device: ``reset()`` zeroes the totals, ``count()`` is the elements
    folded per resolution, ``value()`` the mean over resolutions of (sum / count) in f64, NaN while any count is 0.
    ``count()`` and ``value()`` synchronise."""

    def _init_totals(self, R, device):
        self._sum = torch.zeros(R, dtype=torch.float64, device=device)
        self._count = torch.zeros(R, dtype=torch.int64, device=device)

    def reset(self):
        self._sum.zero_()
        self._count.zero_()
        return self

    def count(self):
        return [int(c) for c in self._count.cpu()]

    def value(self):
        s, c = self._sum.cpu().numpy(), self._count.cpu().numpy()
        if (c == 0).any():
            return float("nan")
        return float(np.mean(s / c))
