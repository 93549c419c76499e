#!/usr/bin/env python3
"""Time MultiMelSpectrogramLoss (adk_mel_distance) against the same computation composed from torch on the GPU.

Shapes: (a) 16 x 9600 samples (the shipped configs' batch_size x batch_length), (b) 256 x 48000 (one second per stream at the
bench's stream count); the vctk config's mel_loss_params (48 kHz, n_fft 2048, hop 300, 80 mels).  Device events after a
warm-up, median of repeats.  FLOP and byte counts come from the shapes:
  FLOP   per frame and signal set: real FFT 2.5 n log2 n + untangle/power/sqrt 12 (n/2 + 1) + mel 2 nnz + log/diff 3 n_mels
  bytes  the two signal sets read once (the torch composition also writes and re-reads its complex spectra)

--backward times forward plus backward instead: the differentiable HIP loss (adk_mel_distance, then adk_mel_distance_grad) against
the torch composition under autograd, y_hat a leaf that requires grad; it also reports the backward's workspace (the slab of
windowed frame gradients) and the relative L2 difference of the two gradients.  A record, not a pass criterion.
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from audiodec_amd import mel, native  # noqa: E402

PARAMS = dict(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048], window="hann_window", num_mels=80, fmin=0,
              fmax=24000, log_base=None)
PEAK_FP32_VECTOR = 157.3e12
SHAPES = {"a": (16, 9600), "b": (256, 48000)}


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def torch_loss(y_hat, y, n_fft, hop, window, melmat_t, eps=1e-10):
    def f(x):
        s = torch.stft(x, n_fft, hop, n_fft, window, return_complex=True)
        amp = torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=eps)).transpose(2, 1)
        return torch.log(torch.clamp(torch.matmul(amp, melmat_t), min=eps)).transpose(1, 2)
    return F.l1_loss(f(y_hat), f(y))


def backward_leg(dev):
    loss = mel.MultiMelSpectrogramLoss(**PARAMS, device=dev, differentiable=True)
    m = loss.mel_transfers[0]
    window = m.window.to(dev)
    melmat_t = torch.from_numpy(m.melmat.T.copy()).to(dev)
    n_fft, hop = m.fft_size, m.hop_size
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, T) in SHAPES.items():
        y = 0.1 * torch.randn(B, T, device=dev, generator=g)
        y_hat = (y + 0.01 * torch.randn(B, T, device=dev, generator=g)).contiguous().requires_grad_(True)

        def hip():
            y_hat.grad = None
            loss(y_hat, y).backward()

        def composed():
            y_hat.grad = None
            torch_loss(y_hat, y, n_fft, hop, window, melmat_t).backward()

        hip_us, torch_us = timed(hip), timed(composed)
        hip()
        g_hip = y_hat.grad.clone()
        composed()
        diff = float((g_hip - y_hat.grad).norm() / y_hat.grad.norm())
        ws = int(native.lib().adk_mel_grad_workspace_bytes(B, T, n_fft, hop))
        row = dict(leg="forward+backward", shape=name, signals=B, samples=T, frames=mel.num_frames(T, hop),
                   hip_us=round(hip_us, 1), torch_us=round(torch_us, 1), speedup=round(torch_us / hip_us, 2),
                   workspace_mb=round(ws / 1e6, 1), grad_rel_l2_diff=diff)
        print(json.dumps(row), flush=True)


def main():
    dev = torch.device("cuda", 0)
    if "--backward" in sys.argv[1:]:
        return backward_leg(dev)
    loss = mel.MultiMelSpectrogramLoss(**PARAMS, device=dev)
    m = loss.mel_transfers[0]
    window = m.window.to(dev)
    melmat_t = torch.from_numpy(m.melmat.T.copy()).to(dev)
    nnz = int(m._weights.size)
    n_fft, hop, n_mels = m.fft_size, m.hop_size, m.num_mels
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name, (B, T) in SHAPES.items():
        y = 0.1 * torch.randn(B, T, device=dev, generator=g)
        y_hat = (y + 0.01 * torch.randn(B, T, device=dev, generator=g)).contiguous()
        frames = mel.num_frames(T, hop)
        flop = 2 * B * frames * (2.5 * n_fft * math.log2(n_fft) + 12 * (n_fft // 2 + 1) + 2 * nnz + 3 * n_mels)
        nbytes = 2 * B * T * 4
        spec_bytes = 2 * B * frames * (n_fft // 2 + 1) * 8
        with torch.no_grad():
            hip_us = timed(lambda: loss(y_hat, y))
            torch_us = timed(lambda: torch_loss(y_hat, y, n_fft, hop, window, melmat_t))
            a, b = float(loss(y_hat, y)), float(torch_loss(y_hat, y, n_fft, hop, window, melmat_t))
        row = dict(shape=name, signals=B, samples=T, frames=frames, hip_us=round(hip_us, 1), torch_us=round(torch_us, 1),
                   speedup=round(torch_us / hip_us, 2), gflop=round(flop / 1e9, 3),
                   fp32_peak_share=round(flop / (hip_us * 1e-6) / PEAK_FP32_VECTOR, 4), input_mb=round(nbytes / 1e6, 1),
                   torch_spectrum_mb=round(spec_bytes / 1e6, 1), loss_hip=a, loss_torch=b)
        rows.append(row)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
