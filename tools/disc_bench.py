#!/usr/bin/env python3
"""Time the HIP discriminator pass + GAN losses against the same network written with F.conv1d / F.conv2d on the GPU.

One eval step of the reference (trainer/autoencoder.py:158-163) at the shipped architecture: B real + B fake rows of T
samples (default 16 + 16 x 48000).  HIP: AdversarialEval.forward (one pass over cat([y_hat, y]), losses folded per layer).
torch: the same weights through F.conv* (MIOpen) in f32, then the reference's loss formulas with torch ops.  Prints one JSON
line: median ms of each, and per-layer GEMM FLOPs for reading a rocprofv3 kernel trace against.

``--backward`` times one generator step's GAN part instead (trainer/autoencoder.py:102-108): D(y) under no_grad, D(y_hat) with the
graph, adversarial_loss, and its backward to y_hat.  HIP: AdversarialEval(differentiable=True) (adk_disc_conv_grad and friends);
torch: the same composition through autograd.  The two are timed alternately after a warm-up of both, each call ending in a device
synchronise; the JSON line also carries the largest difference between the two gradients.

    python tools/disc_bench.py [--batch 16] [--samples 48000] [--iters 5] [--backward]
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


def torch_features(d, ws, x):
    """The reference's forward with torch ops: the list per sub-discriminator of lists of feature maps."""
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
    return outs


def torch_pass(d, ws, x, cfg):
    """The reference's forward and losses with torch ops: (adv, fm, real, fake) as 0-d tensors."""
    n = x.shape[0] // 2
    outs = torch_features(d, ws, x)
    adv = sum(F.mse_loss(o[-1][:n], torch.ones_like(o[-1][:n])) for o in outs)
    fm = sum(sum(F.l1_loss(t[:n], t[n:]) for t in o[:-1]) for o in outs)
    real = sum(F.mse_loss(o[-1][n:], torch.ones_like(o[-1][n:])) for o in outs)
    fake = sum(F.mse_loss(o[-1][:n], torch.zeros_like(o[-1][:n])) for o in outs)
    return cfg["lambda_adv"] * (adv + cfg["lambda_feat_match"] * fm), fm, real, fake


def torch_step(d, ws, y_hat, y, cfg):
    """The generator step's GAN part with torch autograd: (adversarial_loss, its gradient with respect to y_hat)."""
    a = y_hat.detach().requires_grad_(True)
    with torch.no_grad():
        p = torch_features(d, ws, y)
    p_ = torch_features(d, ws, a)
    adv = sum(F.mse_loss(o[-1], torch.ones_like(o[-1])) for o in p_)
    fm = sum(sum(F.l1_loss(t, u) for t, u in zip(oh[:-1], o[:-1])) for oh, o in zip(p_, p))
    loss = cfg["lambda_adv"] * (adv + cfg["lambda_feat_match"] * fm)
    loss.backward()
    return loss.detach(), a.grad


def hip_step(ev, y_hat, y):
    a = y_hat.detach().requires_grad_(True)
    loss = ev(a, y)["adversarial_loss"]
    loss.backward()
    return loss.detach(), a.grad


def backward_bench(a, d_params, sd, ws, cfg, y_hat, y, dev):
    from audiodec_amd import discriminator as D
    d = D.Discriminator(**d_params, device=dev, differentiable=True).load_state_dict(sd)
    ev = D.from_config(cfg, d, differentiable=True)
    steps = {"hip": lambda: hip_step(ev, y_hat, y), "torch": lambda: torch_step(d, ws, y_hat, y, cfg)}
    res, ts = {}, {k: [] for k in steps}
    for k, fn in steps.items():                     # warm-up: code objects, MIOpen's algorithm choice, the backward weight packing
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
    gh, gt = res["hip"][1], res["torch"][1]
    flops = layer_flops(d, a.samples)
    total = sum(flops.values()) * a.batch * 4       # forward of y and of y_hat, and a backward-data pass of the forward's size
    return {"mode": "backward", "batch": a.batch, "samples": a.samples, "iters": a.iters,
            "hip_ms": round(med["hip"], 3), "torch_ms": round(med["torch"], 3), "speedup": round(med["torch"] / med["hip"], 3),
            "hip_ms_min_max": [round(min(ts["hip"]), 3), round(max(ts["hip"]), 3)],
            "torch_ms_min_max": [round(min(ts["torch"]), 3), round(max(ts["torch"]), 3)],
            "tflop": round(total / 1e12, 3), "hip_tflops": round(total / med["hip"] / 1e9, 2),
            "loss": {"hip": float(res["hip"][0]), "torch": float(res["torch"][0])},
            "grad_max_abs": float(gt.abs().max()), "grad_max_diff": float((gh - gt).abs().max())}


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
    ap.add_argument("--backward", action="store_true", help="time forward + backward of adversarial_loss to y_hat")
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
    if a.backward:
        print(json.dumps(backward_bench(a, DO.PARAMS["v1"], sd, ws, cfg, y_hat, y, dev)))
        return
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
