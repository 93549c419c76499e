#!/usr/bin/env python3
"""Generate tests/golden/encoder_grad.npz: known answers of the reference encoder + projector's forward, of its backward to the
input and of its gradients with respect to every parameter.

Runs only where the reference is available.  It imports the UNMODIFIED reference the way make_golden.py does and builds its
``Generator`` from the seeded synthetic weights (audiodec_amd/synth.py), in .eval().

Per case ``projector(encoder(x))`` (models/autoencoder/AudioDec.py:106-108) runs in f32 and, as a deep copy, in f64.  x is
``synth.synth_audio(seed, b * C + c, T)`` per row, the upstream gradient is ``default_rng(seed).standard_normal(z.shape)`` in f32.
Stored, with TENSORS = ("z", "x") + the parameter names in ``named_parameters()`` order:
  * ``{case}_z64``, ``{case}_gx64``: the f64 latent and the f64 gradient with respect to x, whole;
  * ``{case}_names``: the parameter names (the generator's state-dict keys);
  * ``{case}_g{i}``: the f64 gradient of parameter i, ``sample()`` of it: whole up to 4096 elements, else flat[::211] (211 is prime
    to every kernel size and channel count, so the samples walk every tap and channel);
  * ``{case}_max``, ``{case}_E_ref``: per TENSORS entry, max |f64| over the WHOLE tensor and the maximum error of the reference's
    own f32 run against it; ``{case}_seed``.
For every tensor the script asserts 4 * E_ref + 1e-6 * max <= 2e-5 * max.  A single dropped tap moves a weight gradient by about
1 / sqrt(B * T_out) of max, 1e-2 here, so the bound the GPU tests use cannot hide one.

Only inputs' seeds and outputs are stored.  The archive is written with fixed member times.
"""
import copy
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from audiodec_amd import configs, synth  # noqa: E402
from make_golden import SEED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "encoder_grad.npz")
STEP, WHOLE = 211, 4096
CAP = 2e-5

# name: (model alias, x shape)
CASES = {
    "ragged": ("vctk_sym", (3, 1, 301)),                # lengths 301 -> 101 -> 26 -> 6 -> 2: every strided conv sees a ragged tail
    "sym": ("vctk_sym", (2, 1, 3300)),
    "stereo": ("test_stereo_sym", (1, 2, 3000)),
}


def case_seed(name):
    return SEED + 1000 * (1 + list(CASES).index(name))


def case_input(name):
    b, c, t = CASES[name][1]
    seed = case_seed(name)
    return np.stack([synth.synth_audio(seed, i, t) for i in range(b * c)]).reshape(b, c, t)


def upstream(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def sample(a):
    flat = np.asarray(a).reshape(-1)
    return flat if flat.size <= WHOLE else flat[::STEP]


def generator_params(model):
    _, enc_tag, _, _, _ = configs.alias(model)
    _, _, pe = configs.experiment(enc_tag)
    return enc_tag, pe


def main():
    import_reference()
    from models.autoencoder.AudioDec import Generator
    torch.set_num_threads(8)
    out = {"seed": np.int64(SEED)}
    for name, (model, shape) in CASES.items():
        enc_tag, pe = generator_params(model)
        g = Generator(**pe)
        g.load_state_dict(synth.synth_state_dict(enc_tag, SEED))
        g.eval()
        seed = case_seed(name)
        out[f"{name}_seed"] = np.int64(seed)
        x_np = case_input(name)
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            enc, proj = copy.deepcopy(g.encoder).to(dt), copy.deepcopy(g.projector).to(dt)
            named = [(f"encoder.{k}", p) for k, p in enc.named_parameters()] + [(f"projector.{k}", p) for k, p in proj.named_parameters()]
            x = torch.from_numpy(x_np).to(dt).requires_grad_(True)
            z = proj(enc(x))
            (z * torch.from_numpy(upstream(seed, tuple(z.shape))).to(dt)).sum().backward()
            res[tag] = ([k for k, _ in named],
                        [z.detach().double().numpy(), x.grad.double().numpy()] + [p.grad.double().numpy() for _, p in named])
        names, t64 = res["64"]
        assert names == res["32"][0]
        mx, er = [], []
        for what, ref, got in zip(["z", "x"] + names, t64, res["32"][1]):
            e, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            assert np.isfinite(ref).all() and m > 0, (name, what)
            assert 4 * e + 1e-6 * m <= CAP * m, (name, what, e, m)
            mx.append(m)
            er.append(e)
        worst = max((4 * e + 1e-6 * m) / m for e, m in zip(er, mx))
        print(f"{name}: x {shape} z {t64[0].shape} {len(names)} parameters, worst bound/max {worst:.2e}")
        out[f"{name}_z64"], out[f"{name}_gx64"] = t64[0], t64[1]
        out[f"{name}_names"] = np.array(names)
        for i, gr in enumerate(t64[2:]):
            out[f"{name}_g{i}"] = np.ascontiguousarray(sample(gr))
        out[f"{name}_max"], out[f"{name}_E_ref"] = np.asarray(mx, np.float64), np.asarray(er, np.float64)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{OUT}: {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
