"""Cases of tests/golden/univ_disc_grad.npz and an fp64 restatement of the gradient of the generator-side GAN loss
``lambda_adv * (gen_adv(D(y_hat)) + lambda_feat_match * feat_match(D(y_hat), D(y)))`` with respect to ``y_hat`` through the
UnivNet discriminator, its weights fixed (trainer/autoencoder.py:102-108).

As disc_grad_oracle (whose loss, decision and bound helpers are used as they are) the restatement is evaluated AT GIVEN
DECISIONS: ``leaky_relu(z)`` becomes ``z * where(mask, 1, slope)`` and ``|d|`` becomes ``sign * d`` with constant tensors.  The
magnitude spectrogram has no discrete decision -- ``|X|`` is differentiated as torch does it, a bin of magnitude 0 passing no
gradient -- so only the LeakyReLU masks and the L1 signs are decisions.
"""
import numpy as np
import torch
import torch.nn.functional as F

import univ_disc_oracle as UO
from audiodec_amd import synth
from audiodec_amd import univnet_discriminator as U
from disc_grad_oracle import (FLAGS, UPSTREAM, _act, _np, decisions, disagreements, eval_config, layer_bounds,  # noqa: F401
                              loss64, margins64)

# case: (params, (B, C, T) of y_hat and of y)
CASES = {
    "t2310": UO.CASES["t2310"],
    "t301": UO.CASES["t301"],
    "t128": UO.CASES["t128"],                 # the 1024-point spectrogram is all zeros: every frame lies in the zero padding
    "overlap": UO.CASES["overlap"],
    "stereo": UO.CASES["stereo"],
    "tmin": UO.CASES["tmin"],
    "b2": ("reduced", (2, 1, 487)),
    "v3": UO.CASES["v3"],
}
FULL_CASES = [c for c, (p, _) in CASES.items() if p != "v3"]           # per-layer bounds and decision counts stored


def inputs(case):
    """(y_hat, y): float32 (B, C, T) each, as univ_disc_oracle.inputs makes them."""
    if case in UO.CASES:
        return UO.inputs(case)
    _, (b, c, t) = CASES[case]
    rows = [synth.synth_audio(UO.SEED, f"univ_disc/{case}/{i}", t) for i in range(2 * b * c)]
    x = np.stack(rows).reshape(2 * b, c, t).astype(np.float32)
    return x[:b], x[b:]


def features64(pname, sd, x, masks=None):
    """univ_disc_oracle.forward64 on a float64 torch tensor x (N, C, T), kept in torch so that autograd can walk it; masks[d][l]
    (bool, the feature map's shape) replaces layer (d, l)'s LeakyReLU decision."""
    p = UO.PARAMS[pname]
    disc = U.Discriminator(**p)
    n, c, t = x.shape
    if c != 1 and p.get("flat_channel", False):
        x = x.reshape(n * c, 1, t)
    outs = []
    for sub in disc.mrsd.discriminators:
        d, o = len(outs), []
        h = UO.spectrogram64(x[:, 0], sd[sub.window_key].double(), sub.fft_size, sub.hop_size, sub.win_length)[:, None]
        for l, L in enumerate(sub.layers):
            w, b = UO._weight64(sd, L)
            h = F.conv2d(h, w, b, stride=L.stride, padding=L.pad)
            h = _act(h, L, None if masks is None else masks[d][l])
            o.append(h)
        outs.append(o)
    for period, layers in zip(p["periods"], disc.mpd.discriminator_layers):
        d, h = len(outs), x
        tt = h.shape[-1]
        if tt % period:
            h = F.pad(h, (0, period - tt % period), "reflect")
        h = h.view(h.shape[0], h.shape[1], -1, period)
        o = []
        for l, L in enumerate(layers):
            w, b = UO._weight64(sd, L)
            h = F.conv2d(h, w, b, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups)
            h = _act(h, L, None if masks is None else masks[d][l])
            o.append(h)
        o[-1] = o[-1].reshape(o[-1].shape[0], -1)
        outs.append(o)
    return outs


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
    """The same gradient by plain fp64 autograd of univ_disc_oracle's formulas (leaky_relu and |.| as torch differentiates them)."""
    with torch.no_grad():
        fr = features64(pname, sd, torch.from_numpy(np.asarray(y)).double())
    x = torch.from_numpy(np.asarray(y_hat)).double().requires_grad_(True)
    loss = loss64(features64(pname, sd, x), flags, feats=fr)
    (UPSTREAM * loss).backward()
    return x.grad.numpy()
