"""Cases of tests/golden/disc_grad.npz and an fp64 restatement of the gradient of the generator-side GAN loss
``lambda_adv * (gen_adv(D(y_hat)) + lambda_feat_match * feat_match(D(y_hat), D(y)))`` with respect to ``y_hat``, the
discriminator's weights fixed (trainer/autoencoder.py:102-108).

LeakyReLU and the L1 term have a discontinuous derivative: a float32 forward may decide an element that sits on a boundary
differently from fp64, and the two gradients then differ by a finite amount that says nothing about the arithmetic.  So the
restatement is evaluated AT GIVEN DECISIONS: ``leaky_relu(z)`` becomes ``z * where(mask, 1, slope)`` and ``|d|`` becomes
``sign * d`` with constant ``mask`` / ``sign`` tensors, and torch's float64 autograd yields the gradient of the loss linearised at
those decisions.  ``decisions`` derives them from any set of feature maps (``a_hat > 0`` and ``sign(a_hat - a)``); with the fp64
feature maps' own decisions the result is plain fp64 autograd of disc_oracle's formulas.
"""
import numpy as np
import torch
import torch.nn.functional as F

import disc_oracle as DO
from audiodec_amd import discriminator as D
from audiodec_amd import synth

# case: (params, (B, C, T) of y_hat and of y)
CASES = {
    "t1203": DO.CASES["t1203"],
    "t11": DO.CASES["t11"],
    "stereo": DO.CASES["stereo"],
    "b2": ("reduced", (2, 1, 487)),
    "v1": DO.CASES["v1"],
}
REDUCED_CASES = [c for c, (p, _) in CASES.items() if p == "reduced"]

# flag set: generator (average_by_discriminators, loss_type), feature matching (average_by_layers, average_by_discriminators,
# include_final_outputs) or None, lambda_adv, lambda_feat_match; "shipped" = the symAD_* configs'
FLAGS = {
    "shipped": dict(gen=(False, "mse"), fm=(False, False, False), lambda_adv=1.0, lambda_feat_match=2.0),
    "hinge_avg": dict(gen=(True, "hinge"), fm=(True, True, True), lambda_adv=1.5, lambda_feat_match=2.0),
    "mse_nofm": dict(gen=(False, "mse"), fm=None, lambda_adv=1.0, lambda_feat_match=2.0),
}
UPSTREAM = 0.37                                     # the gradient is that of UPSTREAM * adversarial_loss


def inputs(case):
    """(y_hat, y): float32 (B, C, T) each, as disc_oracle.inputs makes them."""
    _, (b, c, t) = CASES[case]
    rows = [synth.synth_audio(DO.SEED, f"disc/{case}/{i}", t) for i in range(2 * b * c)]
    x = np.stack(rows).reshape(2 * b, c, t).astype(np.float32)
    return x[:b], x[b:]


def eval_config(flags):
    """AdversarialEval / from_config arguments of a flag set."""
    f = FLAGS[flags] if isinstance(flags, str) else flags
    cfg = {"generator_adv_loss_params": {"average_by_discriminators": f["gen"][0], "loss_type": f["gen"][1]},
           "discriminator_adv_loss_params": {"average_by_discriminators": f["gen"][0], "loss_type": f["gen"][1]},
           "use_feat_match_loss": f["fm"] is not None, "lambda_adv": f["lambda_adv"], "lambda_feat_match": f["lambda_feat_match"]}
    if f["fm"] is not None:
        cfg["feat_match_loss_params"] = {"average_by_layers": f["fm"][0], "average_by_discriminators": f["fm"][1],
                                         "include_final_outputs": f["fm"][2]}
    return cfg


def _act(h, L, mask):
    if L.act_slope is None:
        return h
    if mask is None:
        return F.leaky_relu(h, L.act_slope)
    m = torch.from_numpy(np.ascontiguousarray(mask)).reshape(h.shape)
    return h * torch.where(m, torch.ones((), dtype=h.dtype), torch.full((), L.act_slope, dtype=h.dtype))


def features64(pname, sd, x, masks=None):
    """disc_oracle.forward64 on a float64 torch tensor x (N, C, T), kept in torch so that autograd can walk it; masks[d][l]
    (bool, the feature map's shape) replaces layer (d, l)'s LeakyReLU decision."""
    p = DO.PARAMS[pname]
    disc = D.Discriminator(**p)
    n, c, t = x.shape
    if c != 1:
        x = x.reshape(n * c, 1, t)
    outs = []
    pool = p["scale_downsample_pooling_params"]
    xs = x
    for layers in disc.msd.discriminator_layers:
        d, h, o = len(outs), xs, []
        for l, L in enumerate(layers):
            w, b = DO._weight64(sd, L)
            h = F.conv1d(h, w, b, stride=L.stride, padding=L.pad, groups=L.groups)
            h = _act(h, L, None if masks is None else masks[d][l])
            o.append(h)
        outs.append(o)
        xs = F.avg_pool1d(xs, pool["kernel_size"], pool["stride"], pool["padding"])
    for period, layers in zip(p["periods"], disc.mpd.discriminator_layers):
        d, h = len(outs), x
        tt = h.shape[-1]
        if tt % period:
            h = F.pad(h, (0, period - tt % period), "reflect")
        h = h.view(h.shape[0], h.shape[1], -1, period)
        o = []
        for l, L in enumerate(layers):
            w, b = DO._weight64(sd, L)
            h = F.conv2d(h, w, b, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups)
            h = _act(h, L, None if masks is None else masks[d][l])
            o.append(h)
        o[-1] = o[-1].reshape(o[-1].shape[0], -1)
        outs.append(o)
    return outs


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def decisions(feats_hat, feats):
    """(masks, signs) of two sets of feature maps (lists per sub-discriminator of lists per layer; arrays or tensors):
    masks[d][l] = a_hat > 0, signs[d][l] = sign(a_hat - a) as float64."""
    masks = [[_np(a) > 0 for a in o] for o in feats_hat]
    signs = [[np.sign(_np(a) - _np(b)).astype(np.float64) for a, b in zip(oh, o)] for oh, o in zip(feats_hat, feats)]
    return masks, signs


def margins64(feats_hat, feats):
    """What an fp64 decision has to spare: (|a_hat|, |a_hat - a|) per layer, of fp64 feature maps."""
    return ([[np.abs(_np(a)) for a in o] for o in feats_hat],
            [[np.abs(_np(a) - _np(b)) for a, b in zip(oh, o)] for oh, o in zip(feats_hat, feats)])


def loss64(feats_hat, flags, signs=None, feats=None):
    """adversarial_loss of a flag set on torch float64 feature maps of y_hat; the L1 terms are sign * (a_hat - a) with the
    given constant signs (and a = 0, which the gradient does not see) or |a_hat - a| with the given natural-side maps."""
    f = FLAGS[flags] if isinstance(flags, str) else flags
    avg, kind = f["gen"]
    adv = sum(torch.mean((o[-1] - 1.0) ** 2) if kind == "mse" else -torch.mean(o[-1]) for o in feats_hat)
    if avg:
        adv = adv / len(feats_hat)
    if f["fm"] is not None:
        by_layers, by_discs, final = f["fm"]
        total = 0.0
        for d, o in enumerate(feats_hat):
            used = range(len(o) if final else len(o) - 1)
            if signs is not None:
                v = sum(torch.mean(torch.from_numpy(np.ascontiguousarray(signs[d][l])).reshape(o[l].shape) * o[l]) for l in used)
            else:
                v = sum(torch.mean(torch.abs(o[l] - torch.as_tensor(_np(feats[d][l])))) for l in used)
            total = total + (v / len(used) if by_layers else v)
        if by_discs:
            total = total / len(feats_hat)
        adv = adv + f["lambda_feat_match"] * total
    return f["lambda_adv"] * adv


def grad64(pname, sd, y_hat, y, flags, masks=None, signs=None):
    """d (UPSTREAM * adversarial_loss) / d y_hat in float64 at the given decisions (default: the fp64 forward's own), as a
    numpy array of y_hat's shape."""
    if masks is None or signs is None:
        with torch.no_grad():
            fh = features64(pname, sd, torch.from_numpy(np.asarray(y_hat)).double())
            fr = features64(pname, sd, torch.from_numpy(np.asarray(y)).double())
        m, s = decisions(fh, fr)
        masks, signs = masks if masks is not None else m, signs if signs is not None else s
    x = torch.from_numpy(np.asarray(y_hat)).double().requires_grad_(True)
    loss = loss64(features64(pname, sd, x, masks), flags, signs=signs)
    (UPSTREAM * loss).backward()
    return x.grad.numpy()


def plain_grad64(pname, sd, y_hat, y, flags):
    """The same gradient by plain fp64 autograd of disc_oracle's formulas (leaky_relu and |.| as torch differentiates them)."""
    with torch.no_grad():
        fr = features64(pname, sd, torch.from_numpy(np.asarray(y)).double())
    x = torch.from_numpy(np.asarray(y_hat)).double().requires_grad_(True)
    loss = loss64(features64(pname, sd, x), flags, feats=fr)
    (UPSTREAM * loss).backward()
    return x.grad.numpy()


def layer_bounds(ref_feats, exact_feats):
    """test_gpu_discriminator._bound per layer: 4 x the reference's f32 error + 1e-6 max(1, max|exact|), of feature maps of
    cat([y_hat, y]); a flat float64 array in (d, l) order."""
    return np.array([4 * np.max(np.abs(_np(r) - _np(e))) + 1e-6 * max(1.0, float(np.max(np.abs(_np(e)))))
                     for o_r, o_e in zip(ref_feats, exact_feats) for r, e in zip(o_r, o_e)])


def disagreements(masks, signs, masks64, signs64, margins, bounds):
    """[(d, l, what, count, worst margin, bound)] of the layers where given decisions differ from the fp64 ones, and whether
    every differing element's fp64 margin is within its layer's bound.  The last layer of a sub-discriminator has no activation:
    its mask is not a decision."""
    out, ok, i = [], True, 0
    for d in range(len(masks64)):
        for l in range(len(masks64[d])):
            for what, got, want, marg in (("mask", masks[d][l], masks64[d][l], margins[0][d][l]),
                                          ("sign", signs[d][l], signs64[d][l], margins[1][d][l])):
                if what == "mask" and l == len(masks64[d]) - 1:
                    continue
                diff = np.asarray(got).reshape(np.shape(want)) != want
                if diff.any():
                    worst = float(marg[diff].max())
                    out.append((d, l, what, int(diff.sum()), worst, float(bounds[i])))
                    ok = ok and worst <= bounds[i]
            i += 1
    return out, ok
