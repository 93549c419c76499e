#!/usr/bin/env python3
"""Time forward + backward (to every parameter and to zq) of the trainable decoder on the HIP path against the same network
written with F.conv1d / F.conv_transpose1d / F.elu and torch autograd on the GPU.

The shipped vctk_sym decoder with the seeded synthetic weights, zq (B, 64, T) (default 16 x 160 frames = 16 x 48000 output
samples), a fixed random upstream gradient on the waveform.  HIP: TrainableDecoder (adk_dec_conv, adk_dec_convtr, their _grad
calls, adk_conv_wgrad and adk_convtr_wgrad).  torch: the same weights through torch's convs (MIOpen) in f32, on the same device.
The two are timed alternately after a warm-up of both, each call ending in a device synchronise.  Prints one JSON line: median and
spread of each, and the largest difference between the two waveforms and between the two sets of gradients (zq's and every
parameter's, relative to each gradient's largest element).

    python tools/dec_train_bench.py [--batch 16] [--frames 160] [--iters 9] [--only hip|torch]

``--only`` runs one leg alone, for a kernel trace of it.
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


def torch_decoder(specs, params, x, alpha):
    """Decoder.forward (decoder.py:135-138) with torch ops; params: name -> tensor."""

    def conv(h, s):
        w, b = params[s.wkey("weight")], params[s.wkey("bias")] if s.bias else None
        if s.kind == "convT":                       # CausalConvTranspose1d.forward (conv_layer.py:189-192)
            return F.conv_transpose1d(F.pad(h, (1, 0), mode="replicate"), w, b, stride=s.stride)[:, :, s.stride:-s.stride]
        return F.conv1d(F.pad(h, ((s.k - 1) * s.dilation, 0)), w, b, dilation=s.dilation)

    x = conv(x, specs[0])
    i = 1
    while i < len(specs) - 1:
        if ".res_units." in specs[i].name:
            x = x + conv(F.elu(conv(F.elu(x, alpha), specs[i]), alpha), specs[i + 1])
            i += 2
        else:
            x = conv(x, specs[i])
            i += 1
    return conv(x, specs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--only", choices=("hip", "torch"))
    a = ap.parse_args()
    from audiodec_amd import configs, synth
    from audiodec_amd import decoder_train as DT
    dev = "cuda:0"
    _, enc_tag, _, _, _ = configs.alias("vctk_sym")
    _, _, pe = configs.experiment(enc_tag)
    dec = DT.TrainableDecoder(**pe)
    dec.load_state_dict(synth.synth_state_dict(enc_tag, 1337))
    dec.to(dev)
    twin = {k: p.detach().clone().requires_grad_(True) for k, p in dec.named_parameters()}
    g = torch.Generator(device=dev).manual_seed(0)
    zq = torch.randn(a.batch, pe["code_dim"], a.frames, device=dev, generator=g).requires_grad_(True)
    up = torch.randn(a.batch, pe["output_channels"], a.frames * dec.hop, device=dev, generator=g)

    def hip():
        dec.zero_grad(set_to_none=True)
        zq.grad = None
        y = dec(zq)
        y.backward(up)
        return y.detach(), [zq.grad] + [p.grad for p in dec.parameters()]

    def ref():
        for p in twin.values():
            p.grad = None
        zq.grad = None
        y = torch_decoder(dec._specs, twin, zq, dec.alpha)
        y.backward(up)
        return y.detach(), [zq.grad] + [p.grad for p in twin.values()]

    steps = {k: fn for k, fn in (("hip", hip), ("torch", ref)) if a.only in (None, k)}
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
    for s in dec._specs:
        t *= s.stride if s.kind == "convT" else 1
        flops += 2 * a.batch * t * s.cout * s.cin * (2 if s.kind == "convT" else s.k)      # a transposed conv's output has two taps
    out = {"batch": a.batch, "frames": a.frames, "iters": a.iters,
           "tflop": round(3 * flops / 1e12, 3),     # the forward, a backward-data and a backward-weight pass of its size
           "saved_mib": round(dec.saved_floats(a.batch, a.frames) * 4 / 2 ** 20, 1)}
    for k in steps:
        out[f"{k}_ms"] = round(med[k], 3)
        out[f"{k}_ms_min_max"] = [round(min(ts[k]), 3), round(max(ts[k]), 3)]
        out[f"{k}_tflops"] = round(3 * flops / med[k] / 1e9, 2)
    if len(steps) == 2:
        out["speedup"] = round(med["torch"] / med["hip"], 3)
        out["y_max_abs"] = float(res["torch"][0].abs().max())
        out["y_max_diff"] = float((res["hip"][0] - res["torch"][0]).abs().max())
        out["grad_max_rel_diff"] = max(float((h - r).abs().max() / r.abs().max()) for h, r in zip(res["hip"][1], res["torch"][1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
