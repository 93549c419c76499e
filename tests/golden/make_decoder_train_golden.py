#!/usr/bin/env python3
"""Generate tests/golden/decoder_train.npz: known answers of the reference decoder's forward, of its backward to the input and of
its gradients with respect to every parameter.

Runs only where the reference is available.  It imports the UNMODIFIED reference the way make_golden.py does and builds its
``Generator`` from the seeded synthetic weights (audiodec_amd/synth.py), in .eval().

Per case the reference ``Decoder`` (models/autoencoder/modules/decoder.py:79-138) runs in f32 and, as a deep copy, in f64.  The
cases, their inputs (slices of a ``zq`` stored in forward.npz), seeds and upstream gradients
(``default_rng(seed).standard_normal(y.shape)`` in f32) are make_decoder_grad_golden.py's.  Stored, with TENSORS = ("y", "zq") +
the parameter names in ``named_parameters()`` order under the generator's ``decoder.`` prefix:
  * ``{case}_y64``, ``{case}_gzq64``: the f64 output and the f64 gradient with respect to zq, whole;
  * ``{case}_names``: the parameter names (the generator's state-dict keys);
  * ``{case}_g{i}``: the f64 gradient of parameter i, ``sample()`` of it: whole up to 4096 elements, else flat[::211] (211 is prime
    to every kernel size and channel count, so the samples walk every tap and channel);
  * ``{case}_max``, ``{case}_E_ref``: per TENSORS entry, max |f64| over the WHOLE tensor and the maximum error of the reference's
    own f32 run against it; ``{case}_seed``, ``{case}_slice``.
For every tensor the script asserts 4 * E_ref + 1e-6 * max <= 5e-5 * max (the worst is a transposed conv's bias, a heavily
cancelling sum).  One dropped tap or phase moves a gradient by at least 1e-2 of max, so the bound the GPU tests use cannot hide one.

Only outputs, seeds and slices are stored.  The archive is written with fixed member times.
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

from audiodec_amd import synth  # noqa: E402
from make_decoder_grad_golden import CASES, case_seed, case_slice, generator_params, upstream  # noqa: E402,F401
from make_golden import SEED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "decoder_train.npz")
STEP, WHOLE = 211, 4096
CAP = 5e-5


def sample(a):
    flat = np.asarray(a).reshape(-1)
    return flat if flat.size <= WHOLE else flat[::STEP]


def case_input(name, fwd=None):
    """The case's zq (B, code_dim, T), f32."""
    _, fcase, sl = CASES[name]
    fwd = fwd if fwd is not None else np.load(os.path.join(HERE, "forward.npz"), allow_pickle=False)
    return case_slice(fwd[f"{fcase}_zq"], sl)


def main():
    import_reference()
    from models.autoencoder.AudioDec import Generator
    torch.set_num_threads(8)
    fwd = np.load(os.path.join(HERE, "forward.npz"), allow_pickle=False)
    out = {"seed": np.int64(SEED)}
    for name, (model, _, sl) in CASES.items():
        enc_tag, pe = generator_params(model)
        g = Generator(**pe)
        g.load_state_dict(synth.synth_state_dict(enc_tag, SEED))
        g.eval()
        seed = case_seed(name)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_slice"] = np.asarray(sl, np.int64)
        zq_np = case_input(name, fwd)
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            dec = copy.deepcopy(g.decoder).to(dt)
            named = [(f"decoder.{k}", p) for k, p in dec.named_parameters()]
            zq = torch.from_numpy(zq_np).to(dt).requires_grad_(True)
            y = dec(zq)
            (y * torch.from_numpy(upstream(seed, tuple(y.shape))).to(dt)).sum().backward()
            res[tag] = ([k for k, _ in named],
                        [y.detach().double().numpy(), zq.grad.double().numpy()] + [p.grad.double().numpy() for _, p in named])
        names, t64 = res["64"]
        assert names == res["32"][0]
        mx, er = [], []
        for what, ref, got in zip(["y", "zq"] + names, t64, res["32"][1]):
            e, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            assert np.isfinite(ref).all() and m > 0, (name, what)
            assert 4 * e + 1e-6 * m <= CAP * m, (name, what, e, m)
            mx.append(m)
            er.append(e)
        worst = max(((4 * e + 1e-6 * m) / m, w) for e, m, w in zip(er, mx, ["y", "zq"] + names))
        print(f"{name}: zq {zq_np.shape} y {t64[0].shape} {len(names)} parameters, worst bound/max {worst[0]:.2e} ({worst[1]})")
        out[f"{name}_y64"], out[f"{name}_gzq64"] = t64[0], t64[1]
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
