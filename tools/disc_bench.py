#!/usr/bin/env python3
"""Time the HIP discriminator pass + GAN losses against the same network written with F.conv1d / F.conv2d on the GPU.

One eval step of the reference (trainer/autoencoder.py:158-163) at the shipped architecture: B real + B fake rows of T
samples (default 16 + 16 x 48000).  HIP: AdversarialEval.forward (one pass over cat([y_hat, y]), losses folded per layer).
torch: the same weights through F.conv* (MIOpen) in f32, then the reference's loss formulas with torch ops.  Prints one JSON
line: median ms of each, and per-layer GEMM FLOPs for reading a rocprofv3 kernel trace against.

    python tools/disc_bench.py [--batch 16] [--samples 48000] [--iters 5]
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def torch_pass(d, ws, x, cfg):
    """The reference's forward and losses with torch ops: (adv, fm, real, fake) as 0-d tensors."""
    n = x.shape[0] // 2
    pool = d.msd.pool
    outs, xs = [], x
    for layers in d.msd.discriminator_layers:
        h, o = xs, []
        for L in layers:
            w, b = ws[L.key]
            h = F.conv1d(h, w, b, stride=L.stride, padding=L.pad, groups=L.groups)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h)
        outs.append(o)
        xs = F.avg_pool1d(xs, pool[0], pool[1], pool[2])
    for p, layers in zip(d.mpd.periods, d.mpd.discriminator_layers):
        h = x
        t = h.shape[-1]
        if t % p:
            h = F.pad(h, (0, p - t % p), "reflect")
        h = h.view(h.shape[0], 1, -1, p)
        o = []
        for L in layers:
            w, b = ws[L.key]
            h = F.conv2d(h, w[..., None], b, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h)
        o[-1] = o[-1].flatten(1)
        outs.append(o)
    adv = sum(F.mse_loss(o[-1][:n], torch.ones_like(o[-1][:n])) for o in outs)
    fm = sum(sum(F.l1_loss(t[:n], t[n:]) for t in o[:-1]) for o in outs)
    real = sum(F.mse_loss(o[-1][n:], torch.ones_like(o[-1][n:])) for o in outs)
    fake = sum(F.mse_loss(o[-1][:n], torch.zeros_like(o[-1][:n])) for o in outs)
    return cfg["lambda_adv"] * (adv + cfg["lambda_feat_match"] * fm), fm, real, fake


def layer_flops(d, t):
    """2 * MACs per layer for one row of t samples (keys as in the state dict)."""
    out = {}
    n = t
    k, s, p = d.msd.pool
    from audiodec_amd import discriminator as D
    for layers in d.msd.discriminator_layers:
        h = n
        for L in layers:
            h = D.conv_out_len(h, L)
            out[L.key] = 2 * h * L.cout * (L.cin // L.groups) * L.kernel
        n = D.pool_out_len(n, k, s, p)
    for per, layers in zip(d.mpd.periods, d.mpd.discriminator_layers):
        h = (t + D.reflect_pad_len(t, per)) // per
        for L in layers:
            h = D.conv_out_len(h, L)
            out[L.key] = 2 * h * per * L.cout * (L.cin // L.groups) * L.kernel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import disc_oracle as DO
    from audiodec_amd import discriminator as D
    dev = "cuda:0"
    sd = DO.state_dict("v1")
    d = D.Discriminator(**DO.PARAMS["v1"], device=dev).load_state_dict(sd)
    ws = {L.key: (D.effective_weight(sd, L).to(dev), sd[L.key + ".bias"].to(dev)) for L in d._layers}
    cfg = {"generator_adv_loss_params": {"average_by_discriminators": False},
           "discriminator_adv_loss_params": {"average_by_discriminators": False}, "use_feat_match_loss": True,
           "feat_match_loss_params": {"average_by_discriminators": False, "average_by_layers": False,
                                      "include_final_outputs": False}, "lambda_adv": 1.0, "lambda_feat_match": 2.0}
    ev = D.from_config(cfg, d)
    g = torch.Generator(device=dev).manual_seed(0)
    y = (0.1 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)).contiguous()
    y_hat = (y + 0.02 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)).contiguous()
    x = torch.cat([y_hat, y])

    def timeit(fn):
        ts = []
        for i in range(a.iters + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], r

    with torch.no_grad():
        hip_ms, hv = timeit(lambda: ev(y_hat, y))
        tor_ms, tv = timeit(lambda: torch_pass(d, ws, x, cfg))
    flops = layer_flops(d, a.samples)
    total = sum(flops.values()) * 2 * a.batch
    res = {"batch": a.batch, "samples": a.samples, "hip_ms": round(hip_ms, 3), "torch_ms": round(tor_ms, 3),
           "speedup": round(tor_ms / hip_ms, 3), "tflop": round(total / 1e12, 3),
           "hip_tflops": round(total / hip_ms / 1e9, 2),
           "hip": {k: float(v) for k, v in hv.items()},
           "torch": dict(zip(["adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss"], [float(v) for v in tv]))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
