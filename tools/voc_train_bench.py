#!/usr/bin/env python3
"""Time forward + backward (to every parameter) of the trainable HiFi-GAN vocoder on the HIP path against the same network written
with F.conv1d(groups=) / F.conv_transpose1d / F.leaky_relu, torch's weight norm and torch autograd on the GPU.

The shipped vctk_v1 vocoder with the seeded synthetic weights, c (B, 64, T) -- default 16 x 32 frames = 16 x 9600 samples, the
reference's stage-2 batch (config/vocoder/*.yaml); --frames 160 is the autoencoder benches' size -- and a fixed random upstream
gradient on the waveform.  HIP: TrainableVocoder (the adk_voc_* calls; weight norm, repeat, normalisation and tanh in torch).
torch: the same parameters through torch's convs (MIOpen) in f32, on the same device.  The two are timed alternately after a
warm-up of both, each call ending in a device synchronise.  Prints one JSON line: median and spread of each, the largest
difference between the two waveforms and between the two sets of gradients (relative to each gradient's largest element), and
``repack_ms``: the time of the weight-norm compositions plus the re-packing of all 34 weights, which a training step pays once
after every optimizer step (it is inside ``hip_ms``: the timed step invalidates the packings as an optimizer would).

    python tools/voc_train_bench.py [--batch 16] [--frames 32] [--iters 9] [--only hip|torch]

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


def torch_vocoder(voc, params, c):
    """Generator.forward (HiFiGAN.py:141-161) with torch ops; params: name -> tensor."""
    specs, ix, slope = voc._specs, voc._index, voc.slope

    def conv(h, i):
        s = specs[i]
        w = torch._weight_norm(params[s.wkey("weight_v")], params[s.wkey("weight_g")], 0) if s.wn else params[s.wkey("weight")]
        b = params[s.wkey("bias")] if s.bias else None
        if s.kind == "convT":                       # CausalConvTranspose1d.forward (conv_layer.py:189-192)
            return F.conv_transpose1d(F.pad(h, (1, 0), mode="replicate"), w, b, stride=s.stride)[:, :, s.stride:-s.stride]
        return F.conv1d(F.pad(h, ((s.k - 1) * s.dilation, 0)), w, b, dilation=s.dilation, groups=s.groups)

    def unit(h, a, b):
        t = conv(F.leaky_relu(h, slope), a)
        return h + (conv(F.leaky_relu(t, slope), b) if b is not None else t)

    if voc.norm:
        c = (c - voc.mean[None, :, None]) / voc.scale[None, :, None]
    h = conv(c, 0)
    for i in range(len(voc.params["upsample_scales"])):
        up, chains, out = voc._stage(i)
        h = conv(F.leaky_relu(h, slope), up)
        if voc.multigroup:
            h = h.repeat(1, voc.groups, 1)
            for a, b in chains[0]:
                h = unit(h, a, b)
            h = conv(h, out)
        else:
            cs = 0.0
            for chain in chains:
                x = h
                for a, b in chain:
                    x = unit(x, a, b)
                cs = cs + x
            h = cs / len(chains)
    return torch.tanh(conv(F.leaky_relu(h, 0.01), ix["output_conv"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--model", default="vctk_v1")
    ap.add_argument("--only", choices=("hip", "torch"))
    a = ap.parse_args()
    from audiodec_amd import configs, synth
    from audiodec_amd import vocoder_train as VT
    dev = "cuda:0"
    _, _, _, dec_tag, _ = configs.alias(a.model)
    _, _, p = configs.experiment(dec_tag)
    voc = VT.TrainableVocoder(**p)
    voc.load_state_dict(synth.synth_state_dict(dec_tag, 1337))
    voc.to(dev)
    twin = {k: q.detach().clone().requires_grad_(True) for k, q in voc.named_parameters()}
    g = torch.Generator(device=dev).manual_seed(0)
    c = torch.randn(a.batch, p["in_channels"], a.frames, device=dev, generator=g)
    up = torch.randn(a.batch, p["out_channels"], a.frames * voc.hop, device=dev, generator=g)

    def stale():
        for layer in voc._layers:                   # what an optimizer step does to the packings
            layer._key = None

    def hip():
        voc.zero_grad(set_to_none=True)
        stale()
        y = voc(c)
        y.backward(up)
        return y.detach(), [q.grad for q in voc.parameters()]

    def ref():
        for q in twin.values():
            q.grad = None
        y = torch_vocoder(voc, twin, c)
        y.backward(up)
        return y.detach(), [q.grad for q in twin.values()]

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
    for s in voc._specs:
        t *= s.stride if s.kind == "convT" else 1
        flops += 2 * a.batch * t * s.cout * (s.cin // s.groups) * (2 if s.kind == "convT" else s.k)
    out = {"model": a.model, "batch": a.batch, "frames": a.frames, "iters": a.iters,
           "tflop": round(3 * flops / 1e12, 3),     # the forward, a backward-data and a backward-weight pass of its size
           "saved_mib": round(voc.saved_floats(a.batch, a.frames) * 4 / 2 ** 20, 1)}
    for k in steps:
        out[f"{k}_ms"] = round(med[k], 3)
        out[f"{k}_ms_min_max"] = [round(min(ts[k]), 3), round(max(ts[k]), 3)]
        out[f"{k}_tflops"] = round(3 * flops / med[k] / 1e9, 2)
    if "hip" in steps:
        rp = []
        for _ in range(a.iters):
            stale()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            voc._weights(True)
            torch.cuda.synchronize()
            rp.append((time.perf_counter() - t0) * 1e3)
        out["repack_ms"] = round(sorted(rp)[len(rp) // 2], 3)
    if len(steps) == 2:
        out["speedup"] = round(med["torch"] / med["hip"], 3)
        out["y_max_abs"] = float(res["torch"][0].abs().max())
        out["y_max_diff"] = float((res["hip"][0] - res["torch"][0]).abs().max())
        out["grad_max_rel_diff"] = max(float((h - r).abs().max() / r.abs().max()) for h, r in zip(res["hip"][1], res["torch"][1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
