#!/usr/bin/env python3
"""Time forward + backward of the frozen symmetric decoder on the HIP path against the same decoder written with
F.conv1d / F.conv_transpose1d / F.elu on the GPU.

The shipped vctk_sym decoder with the seeded synthetic weights, zq (B, 64, T) (default 16 x 160 frames = 16 x 48000 samples),
a fixed random upstream gradient on the waveform.  HIP: FrozenDecoder (adk_dec_conv, adk_dec_convtr and their _grad calls).
torch: the same weights through torch's convs (MIOpen) in f32 and torch autograd, on the same device.  The two are timed
alternately after a warm-up of both, each call ending in a device synchronise.  Prints one JSON line: median and spread of each,
and the largest difference between the two outputs and the two gradients.

    python tools/dec_grad_bench.py [--batch 16] [--frames 160] [--iters 7]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def torch_decoder(host, x):
    """Decoder.forward (decoder.py:119-124) with torch ops; host: FrozenDecoder's (spec, weight, bias) list on the device."""
    i, n = 0, len(host)

    def conv(h, spec, w, b):
        return F.conv1d(F.pad(h, ((spec.k - 1) * spec.dilation, 0)), w, b, dilation=spec.dilation)

    x = conv(x, *host[0])
    i = 1
    while i < n - 1:
        spec, w, b = host[i]
        x = F.conv_transpose1d(F.pad(x, (1, 0), mode="replicate"), w, b, stride=spec.stride)[:, :, spec.stride:-spec.stride]
        i += 1
        while i < n - 1 and host[i][0].kind != "convT":
            y = conv(F.elu(x), *host[i])
            x = x + conv(F.elu(y), *host[i + 1])
            i += 2
    return conv(x, *host[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    from audiodec_amd import configs, synth
    from audiodec_amd import decoder_grad as DG
    dev = "cuda:0"
    _, enc_tag, _, _, _ = configs.alias("vctk_sym")
    _, _, pe = configs.experiment(enc_tag)
    dec = DG.FrozenDecoder(pe["code_dim"], pe["output_channels"], pe["decode_channels"], pe["dec_ratios"], pe["dec_strides"],
                           device=dev).load_state_dict(synth.synth_state_dict(enc_tag, 1337))
    host = [(s, w.to(dev), b.to(dev) if b is not None else None) for s, w, b in dec._host]
    g = torch.Generator(device=dev).manual_seed(0)
    zq = torch.randn(a.batch, pe["code_dim"], a.frames, device=dev, generator=g)
    up = torch.randn(a.batch, pe["output_channels"], a.frames * dec.hop, device=dev, generator=g)

    def step(fn):
        x = zq.detach().requires_grad_(True)
        y = fn(x)
        y.backward(up)
        return y.detach(), x.grad

    steps = {"hip": lambda: step(dec), "torch": lambda: step(lambda x: torch_decoder(host, x))}
    res, ts = {}, {k: [] for k in steps}
    for k, fn in steps.items():                     # warm-up: code objects, MIOpen's algorithm choice
        for _ in range(2):
            res[k] = fn()
        torch.cuda.synchronize()
    for _ in range(a.iters):                        # alternate, so that drift of the shared host hits both alike
        for k, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    flops, t = 0, a.frames
    for s, _, _ in dec._host:
        t *= s.stride if s.kind == "convT" else 1
        flops += 2 * a.batch * t * s.cout * s.cin * (2 if s.kind == "convT" else s.k)
    total = 2 * flops                               # the forward, and a backward-data pass of the forward's size
    print(json.dumps({
        "batch": a.batch, "frames": a.frames, "iters": a.iters,
        "hip_ms": round(med["hip"], 3), "torch_ms": round(med["torch"], 3), "speedup": round(med["torch"] / med["hip"], 3),
        "hip_ms_min_max": [round(min(ts["hip"]), 3), round(max(ts["hip"]), 3)],
        "torch_ms_min_max": [round(min(ts["torch"]), 3), round(max(ts["torch"]), 3)],
        "tflop": round(total / 1e12, 3), "hip_tflops": round(total / med["hip"] / 1e9, 2),
        "saved_mib": round(dec.saved_floats(a.batch, a.frames) * 4 / 2 ** 20, 1),
        "y_max_abs": float(res["torch"][0].abs().max()), "y_max_diff": float((res["hip"][0] - res["torch"][0]).abs().max()),
        "grad_max_abs": float(res["torch"][1].abs().max()), "grad_max_diff": float((res["hip"][1] - res["torch"][1]).abs().max())}))


if __name__ == "__main__":
    main()
