#!/usr/bin/env python3
"""Time the discriminator's own update on the HIP path against the same network written with F.conv1d / F.conv2d /
F.leaky_relu / F.avg_pool1d, torch's weight norm and torch autograd on the GPU.

The step is the reference's (trainer/trainerGAN.py:256-294, trainer/autoencoder.py:117-126): ``D(y_)``, ``D(x)``,
``real_loss + fake_loss``, ``zero_grad``, ``backward``, ``clip_grad_norm_``, Adam's ``step``.  The shipped discriminator
(disc_oracle.V1 is every shipped config's ``discriminator_params``) with the seeded synthetic weights, y_ and x (B, 1, T) --
default 16 + 16 x 9600 samples, the reference's batch -- and the shipped mse loss.  HIP: TrainableDiscriminator and its
DiscriminatorAdversarialLoss (the adk_disc_* calls; the weight-norm composition in torch).  torch: copies of the same parameters
through torch's convs (MIOpen) in f32, on the same device.  Each leg owns an Adam optimizer; the optimizer step is inside the
timed region, so the HIP leg re-packs its weights in every iteration, as training does.  The two are timed alternately after a
warm-up of both, each call ending in a device synchronise.  Prints one JSON line: median and spread of each, and, from the first
warm-up step (where both legs still hold the same weights), the two losses and the largest difference between the two sets of
gradients relative to each gradient's largest element.

    python tools/disc_train_bench.py [--batch 16] [--samples 9600] [--iters 9] [--only hip|torch]

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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def torch_discriminator(disc, params, x):
    """Discriminator.forward (HiFiGAN.py:378-395) with torch ops; params: name -> tensor.  Returns the final outputs."""
    def weight(L):
        if L.norm == "weight":
            return torch._weight_norm(params[f"{L.key}.weight_v"], params[f"{L.key}.weight_g"], 0)
        return params[f"{L.key}.weight"]

    def act(h, L):
        return F.leaky_relu(h, L.act_slope) if L.act_slope is not None else h

    b, c, t = x.shape
    if c != 1:
        x = x.reshape(b * c, 1, t)
    finals, xs = [], x
    k, s, p = disc._pool
    for d, layers in enumerate(disc._scale_layers):
        h = xs
        for L in layers:
            h = act(F.conv1d(h, weight(L), params[f"{L.key}.bias"] if L.bias else None, stride=L.stride, padding=L.pad, groups=L.groups), L)
        finals.append(h)
        if d + 1 < len(disc._scale_layers):
            xs = F.avg_pool1d(xs, k, s, p)
    for period, layers in zip(disc._periods, disc._period_layers):
        h = x
        if t % period:
            h = F.pad(h, (0, period - t % period), "reflect")
        h = h.view(h.shape[0], h.shape[1], -1, period)
        for L in layers:
            h = act(F.conv2d(h, weight(L), params[f"{L.key}.bias"], stride=(L.stride, 1), padding=(L.pad, 0)), L)
        finals.append(torch.flatten(h, 1, -1))
    return finals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=9600)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--only", choices=("hip", "torch"))
    a = ap.parse_args()
    if a.iters < 7:
        ap.error("--iters must be at least 7")
    import disc_oracle as DO
    from audiodec_amd import discriminator_train as T
    dev = "cuda:0"
    disc = T.TrainableDiscriminator(**DO.V1)
    disc.load_state_dict(DO.state_dict("v1"))
    disc.to(dev)
    twin = {k: q.detach().clone().requires_grad_(True) for k, q in disc.named_parameters()}
    g = torch.Generator(device=dev).manual_seed(0)
    y_ = 0.3 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)
    x = 0.3 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)
    crit = T.DiscriminatorAdversarialLoss(average_by_discriminators=False, loss_type="mse")
    adam = dict(lr=2.0e-4, betas=(0.5, 0.9))
    opts = {"hip": torch.optim.Adam(disc.parameters(), **adam), "torch": torch.optim.Adam(twin.values(), **adam)}
    clip = 10.0

    def hip():
        real, fake = crit(disc(y_), disc(x))
        opts["hip"].zero_grad()
        (real + fake).backward()
        grads = [q.grad.clone() for q in disc.parameters()] if keep else None
        torch.nn.utils.clip_grad_norm_(disc.parameters(), clip)
        opts["hip"].step()
        return (real + fake).detach(), grads

    def ref():
        fake = sum(torch.mean(o ** 2) for o in torch_discriminator(disc, twin, y_))
        real = sum(torch.mean((o - 1.0) ** 2) for o in torch_discriminator(disc, twin, x))
        opts["torch"].zero_grad()
        (real + fake).backward()
        grads = [q.grad.clone() for q in twin.values()] if keep else None
        torch.nn.utils.clip_grad_norm_(twin.values(), clip)
        opts["torch"].step()
        return (real + fake).detach(), grads

    steps = {k: fn for k, fn in (("hip", hip), ("torch", ref)) if a.only in (None, k)}
    first, ts = {}, {k: [] for k in steps}
    for k, fn in steps.items():                     # warm-up: code objects, MIOpen's algorithm choice; the first step is compared
        keep = True
        first[k] = fn()
        keep = False
        fn()
        torch.cuda.synchronize()
    for _ in range(a.iters):                        # alternate, so that drift of the shared host hits both alike
        for k, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    out = {"batch": a.batch, "samples": a.samples, "iters": a.iters, "parameters": sum(q.numel() for q in disc.parameters())}
    for k in steps:
        out[f"{k}_ms"] = round(med[k], 3)
        out[f"{k}_ms_min_max"] = [round(min(ts[k]), 3), round(max(ts[k]), 3)]
        out[f"{k}_first_loss"] = float(first[k][0])
    if len(steps) == 2:
        out["speedup"] = round(med["torch"] / med["hip"], 3)
        out["grad_max_rel_diff"] = max(float((h - r).abs().max() / r.abs().max()) for h, r in zip(first["hip"][1], first["torch"][1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
