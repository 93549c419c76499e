#!/usr/bin/env python3
"""Time the HIP UnivNet discriminator pass + GAN losses against the same network composed from torch.stft + F.conv2d.

One eval step of the reference at the shipped parameters: B real + B fake rows of T samples (default 16 + 16 x 48000).
HIP: AdversarialEval.forward (one pass over cat([y_hat, y]), losses folded per layer).  torch: the same weights through
torch.stft / F.conv2d (MIOpen) in f32, then the reference's loss formulas with torch ops.  The two legs alternate in one
process after warm-up and are timed with device events.  Prints one JSON line: the median ms of each leg, the spread of the
torch leg, and per-layer FLOPs of the spectral half for reading a rocprofv3 kernel trace against.

``--backward`` times one generator step's GAN part instead (trainer/autoencoder.py:102-108): D(y) under no_grad, D(y_hat) with the
graph, adversarial_loss, and its backward to y_hat.  HIP: AdversarialEval(differentiable=True) on a DifferentiableDiscriminator
(adk_spectrogram_grad, adk_conv2d_grad, adk_disc_conv_grad and friends).  torch: autograd through the same composition.  After a
warm-up the two legs alternate, each call ending in a device synchronise; the JSON line has each leg's median and min / max.

    python tools/univ_disc_bench.py [--batch 16] [--samples 48000] [--iters 7] [--hip-only] [--backward]
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
    """The reference's forward with torch ops: the list (per sub-discriminator) of lists of feature maps."""
    outs = []
    for sub in d.mrsd.discriminators:
        pad = sub.win_length // 2
        s = torch.stft(F.pad(x[:, 0], (pad, pad)), sub.fft_size, sub.hop_size, sub.win_length, ws[sub.window_key], center=True,
                       pad_mode="reflect", normalized=False, onesided=True, return_complex=True).abs()
        h, o = s.transpose(-1, -2)[:, None], []
        for L in sub.layers:
            w, b = ws[L.key]
            h = F.conv2d(h, w, b, stride=L.stride, padding=L.pad)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h)
        outs.append(o)
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


def backward_bench(a, sd, ws, cfg, y_hat, y, dev):
    import univ_disc_oracle as UO
    from audiodec_amd import univnet_discriminator as U
    d = U.DifferentiableDiscriminator(**UO.PARAMS["v3"], device=dev).load_state_dict(sd)
    ev = U.from_config(cfg, d, differentiable=True)
    steps = {"hip": lambda: hip_step(ev, y_hat, y)}
    if not a.hip_only:
        steps["torch"] = lambda: torch_step(d, ws, y_hat, y, cfg)
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
    out = {"mode": "backward", "batch": a.batch, "samples": a.samples, "iters": a.iters, "hip_ms": round(med["hip"], 3),
           "hip_ms_min_max": [round(min(ts["hip"]), 3), round(max(ts["hip"]), 3)], "loss": {"hip": float(res["hip"][0])},
           "grad_finite": bool(torch.isfinite(res["hip"][1]).all())}
    if not a.hip_only:
        gh, gt = res["hip"][1], res["torch"][1]
        out.update({"torch_ms": round(med["torch"], 3), "torch_ms_min_max": [round(min(ts["torch"]), 3), round(max(ts["torch"]), 3)],
                    "torch_spread_ms": round(max(ts["torch"]) - min(ts["torch"]), 3), "speedup": round(med["torch"] / med["hip"], 3),
                    "grad_max_abs": float(gt.abs().max()), "grad_max_diff": float((gh - gt).abs().max())})
        out["loss"]["torch"] = float(res["torch"][0])
    return out


def spectral_flops(d, t):
    """2 * MACs per spectral layer, and the frame count per spectrogram, for one row of t samples."""
    from audiodec_amd import univnet_discriminator as U
    out = {}
    for sub in d.mrsd.discriminators:
        frames, _ = U.spectrogram_shape(t, sub.fft_size, sub.hop_size, sub.win_length)
        out[sub.window_key] = {"frames": frames, "n_fft": sub.fft_size}
        for L, (_, c, ho, wo) in zip(sub.layers, sub.output_shapes(1, t)):
            out[L.key] = 2 * c * ho * wo * L.cin * L.kernel[0] * L.kernel[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--hip-only", action="store_true", help="run only the HIP leg (for a kernel trace of its own)")
    ap.add_argument("--backward", action="store_true", help="time forward + backward of adversarial_loss to y_hat")
    a = ap.parse_args()
    import univ_disc_oracle as UO
    from audiodec_amd import univnet_discriminator as U
    dev = "cuda:0"
    sd = UO.state_dict("v3")
    d = U.Discriminator(**UO.PARAMS["v3"], device=dev).load_state_dict(sd)
    ws = {L.key: (U.effective_weight(sd, L).to(dev), sd[L.key + ".bias"].to(dev)) for L in d._layers}
    ws.update({k: sd[k].to(dev) for k, _, _, _ in d._specs})
    cfg = {"generator_adv_loss_params": {"average_by_discriminators": False},
           "discriminator_adv_loss_params": {"average_by_discriminators": False}, "use_feat_match_loss": True,
           "feat_match_loss_params": {"average_by_discriminators": False, "average_by_layers": False,
                                      "include_final_outputs": False}, "lambda_adv": 1.0, "lambda_feat_match": 2.0}
    ev = U.from_config(cfg, d)
    g = torch.Generator(device=dev).manual_seed(0)
    y = (0.1 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)).contiguous()
    y_hat = (y + 0.02 * torch.randn(a.batch, 1, a.samples, device=dev, generator=g)).contiguous()
    if a.backward:
        print(json.dumps(backward_bench(a, sd, ws, cfg, y_hat, y, dev)))
        return
    x = torch.cat([y_hat, y])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    legs = {"hip": lambda: ev(y_hat, y)}
    if not a.hip_only:
        legs["torch"] = lambda: torch_pass(d, ws, x, cfg)
    ms = {k: [] for k in legs}
    vals = {}
    with torch.no_grad():
        for i in range(a.iters + 2):                          # two warm-up rounds, then alternating
            for k, fn in legs.items():
                t, vals[k] = timed(fn)
                if i >= 2:
                    ms[k].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    flops = spectral_flops(d, a.samples)
    spectral = sum(v for v in flops.values() if not isinstance(v, dict)) * 2 * a.batch
    res = {"batch": a.batch, "samples": a.samples, "hip_ms": round(med["hip"], 3), "hip_ms_all": [round(t, 3) for t in ms["hip"]],
           "spectral_tflop": round(spectral / 1e12, 4), "layer_flops_per_row": flops,
           "hip": {k: float(v) for k, v in vals["hip"].items()}}
    if not a.hip_only:
        res.update({"torch_ms": round(med["torch"], 3), "torch_ms_all": [round(t, 3) for t in ms["torch"]],
                    "torch_spread_ms": round(max(ms["torch"]) - min(ms["torch"]), 3), "speedup": round(med["torch"] / med["hip"], 3),
                    "torch": dict(zip(["adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss"],
                                      [float(v) for v in vals["torch"]]))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
