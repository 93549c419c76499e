#!/usr/bin/env python3
"""Time MultiResolutionSTFTLoss (adk_stft_distance) and MultiWindowShapeLoss (adk_shape_distance) against the same
computations composed from torch on the GPU.

Shapes: (a) 16 x 9600 samples (the shipped configs' batch_size x batch_length), (b) 256 x 48000 (one second per stream at the
bench's stream count); the shipped configs' stft_loss_params (1024/2048/512, 120/240/50, 600/1200/240) and winlen [300].
Device events after 5 warm-up runs, median of 20.  FLOP and byte counts come from the shapes:
  FLOP   per frame and signal set: real FFT 2.5 n log2 n + untangle/power/sqrt 12 (n/2 + 1); per bin pair 8 (difference, two
         squares, two logs counted as one each, difference, abs, three adds)
  bytes  the two signal sets read once per resolution (the torch composition also writes and re-reads its complex spectra and
         magnitudes)
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from audiodec_amd import stft_loss, waveform_loss  # noqa: E402

PARAMS = dict(fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window")
WINLEN = [300]
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


def torch_stft_loss(x, y, windows, eps=1e-7):
    def mag(s, n_fft, hop, wl, window):
        z = torch.stft(s, n_fft, hop, wl, window, return_complex=True)
        return torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=eps)).transpose(2, 1)
    sc = mg = 0.0
    for (n_fft, hop, wl), window in zip(zip(PARAMS["fft_sizes"], PARAMS["hop_sizes"], PARAMS["win_lengths"]), windows):
        xm, ym = mag(x, n_fft, hop, wl, window), mag(y, n_fft, hop, wl, window)
        sc = sc + torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro")
        mg = mg + F.l1_loss(torch.log(ym), torch.log(xm))
    return sc / len(windows), mg / len(windows)


def torch_shape_loss(y_hat, y):
    total = 0.0
    for w in WINLEN:
        total = total + F.l1_loss(F.max_pool1d(y_hat.abs()[:, None], w), F.max_pool1d(y.abs()[:, None], w))
    return total / len(WINLEN)


def main():
    dev = torch.device("cuda", 0)
    loss = stft_loss.MultiResolutionSTFTLoss(**PARAMS, device=dev)
    shape = waveform_loss.MultiWindowShapeLoss(WINLEN)
    windows = [f.window.to(dev) for f in loss.stft_losses]
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, T) in SHAPES.items():
        y = 0.1 * torch.randn(B, T, device=dev, generator=g)
        y_hat = (y + 0.01 * torch.randn(B, T, device=dev, generator=g)).contiguous()
        flop = 0.0
        spec_bytes = 0
        for n_fft, hop in zip(PARAMS["fft_sizes"], PARAMS["hop_sizes"]):
            frames, bins = stft_loss.num_frames(T, hop), n_fft // 2 + 1
            flop += 2 * B * frames * (2.5 * n_fft * math.log2(n_fft) + 12 * bins) + 8 * B * frames * bins
            spec_bytes += 2 * B * frames * bins * 8
        with torch.no_grad():
            hip_us = timed(lambda: loss(y_hat, y))
            torch_us = timed(lambda: torch_stft_loss(y_hat, y, windows))
            a, b = loss(y_hat, y), torch_stft_loss(y_hat, y, windows)
            row = dict(loss="stft", shape=name, signals=B, samples=T, hip_us=round(hip_us, 1), torch_us=round(torch_us, 1),
                       speedup=round(torch_us / hip_us, 2), gflop=round(flop / 1e9, 3),
                       fp32_peak_share=round(flop / (hip_us * 1e-6) / PEAK_FP32_VECTOR, 4),
                       input_mb=round(3 * 2 * B * T * 4 / 1e6, 1), torch_spectrum_mb=round(spec_bytes / 1e6, 1),
                       sc_hip=float(a[0]), sc_torch=float(b[0]), mag_hip=float(a[1]), mag_torch=float(b[1]))
            print(json.dumps(row), flush=True)
            hip_us = timed(lambda: shape(y_hat, y))
            torch_us = timed(lambda: torch_shape_loss(y_hat, y))
            row = dict(loss="shape", shape=name, signals=B, samples=T, winlen=WINLEN, hip_us=round(hip_us, 1),
                       torch_us=round(torch_us, 1), speedup=round(torch_us / hip_us, 2), input_mb=round(2 * B * T * 4 / 1e6, 1),
                       gbytes_per_s=round(2 * B * T * 4 / (hip_us * 1e-6) / 1e9, 1),
                       loss_hip=float(shape(y_hat, y)), loss_torch=float(torch_shape_loss(y_hat, y)))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
