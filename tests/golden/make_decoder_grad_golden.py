#!/usr/bin/env python3
"""Generate tests/golden/decoder_grad.npz: known answers of the reference decoder's forward and backward to its input, and
of the quantizer's straight-through gradient.

Runs only where the reference is available.  It imports the UNMODIFIED reference the way make_golden.py does and builds its
``Generator`` from the seeded synthetic weights (audiodec_amd/synth.py), in .eval().

Per decoder case the reference ``Decoder`` (models/autoencoder/modules/decoder.py:79-138) runs in f32 and, as a deep copy, in
f64.  The input is a slice of a ``zq`` stored in forward.npz, the upstream gradient is
``default_rng(seed).standard_normal(y.shape)`` in f32.  Stored:
  * ``{case}_y64``, ``{case}_grad64``: the f64 output and the f64 gradient with respect to the input, whole;
  * ``{case}_E_ref_y``, ``{case}_E_ref_g``: the maximum error of the reference's own f32 run against them;
  * ``{case}_max_y``, ``{case}_max_g``: max |y64|, max |grad64|; ``{case}_seed``; ``{case}_slice`` = (b0, b1, t0, t1).
For every case the script asserts 4 * E_ref + 1e-6 * max <= 1e-5 * max: the bound the GPU tests use cannot hide a wrong tap.

Per quantizer case (the ``z`` slices that match the decoder cases) the reference ``Quantizer.forward`` (quantizer.py:32-35) gives
``z.grad`` of ``(zq * up).sum() + (vqloss * w).sum()``, up = default_rng(seed + 1).standard_normal(zq.shape) in f32, w = 1..n_q:
  * ``{case}_q_grad`` f32, and ``{case}_q_idx0`` int16, the stage-0 code of every row (b, t), which the closed form
    dz = up + w[0] * 2 * (z - q0) / (rows * dim) needs.

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

from audiodec_amd import configs, synth  # noqa: E402
from make_golden import SEED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "decoder_grad.npz")

# name: (model alias, forward.npz case, (b0, b1, t0, t1))
CASES = {
    "sym": ("vctk_sym", "b3", (0, 2, 0, 11)),
    "stereo": ("test_stereo_sym", "stereo", (0, 1, 0, 10)),
    "frame1": ("vctk_sym", "b3", (0, 3, 0, 1)),         # every transposed conv sees only its replicate padding
}


def case_seed(name):
    return SEED + 100 * (1 + list(CASES).index(name))


def case_slice(arr, sl):
    b0, b1, t0, t1 = sl
    return np.ascontiguousarray(arr[b0:b1, :, t0:t1])


def upstream(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def generator_params(model):
    _, enc_tag, _, _, _ = configs.alias(model)
    _, _, pe = configs.experiment(enc_tag)
    return enc_tag, pe


def main():
    import_reference()
    from models.autoencoder.AudioDec import Generator
    torch.set_num_threads(4)
    fwd = np.load(os.path.join(HERE, "forward.npz"), allow_pickle=False)
    out = {"seed": np.int64(SEED)}
    for name, (model, fcase, sl) in CASES.items():
        enc_tag, pe = generator_params(model)
        g = Generator(**pe)
        g.load_state_dict(synth.synth_state_dict(enc_tag, SEED))
        g.eval()
        seed = case_seed(name)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_slice"] = np.asarray(sl, np.int64)

        # decoder
        zq = case_slice(fwd[f"{fcase}_zq"], sl)
        dec32, dec64 = g.decoder, copy.deepcopy(g.decoder).double()
        res = {}
        for tag, dec, dt in (("32", dec32, torch.float32), ("64", dec64, torch.float64)):
            x = torch.from_numpy(zq).to(dt).requires_grad_(True)
            y = dec(x)
            up = torch.from_numpy(upstream(seed, tuple(y.shape))).to(dt)
            (y * up).sum().backward()
            res[tag] = (y.detach().double().numpy(), x.grad.double().numpy())
        y64, g64 = res["64"]
        for k, ref, got in (("y", y64, res["32"][0]), ("g", g64, res["32"][1])):
            e, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            out[f"{name}_E_ref_{k}"], out[f"{name}_max_{k}"] = np.float64(e), np.float64(m)
            assert 4 * e + 1e-6 * m <= 1e-5 * m, (name, k, e, m)
            print(f"decoder {name} {k}: shape {ref.shape} E_ref {e:.2e} max {m:.3f} bound/max {(4 * e + 1e-6 * m) / m:.2e}")
        assert np.isfinite(g64).all() and np.abs(g64).max() > 0
        out[f"{name}_y64"], out[f"{name}_grad64"] = y64, g64

        # quantizer
        z = torch.from_numpy(case_slice(fwd[f"{fcase}_z"], sl)).requires_grad_(True)
        zq_t, vqloss, _ = g.quantizer(z)
        n_q = vqloss.numel()
        upq = torch.from_numpy(upstream(seed + 1, tuple(zq_t.shape)))
        w = torch.arange(1, n_q + 1, dtype=torch.float32)
        ((zq_t * upq).sum() + (vqloss * w).sum()).backward()
        with torch.no_grad():
            _, idx = g.quantizer.codebook.layers[0].forward_index(z.detach().transpose(2, 1))
        out[f"{name}_q_grad"] = z.grad.numpy().astype(np.float32)
        out[f"{name}_q_idx0"] = idx.numpy().astype(np.int16)
        print(f"quantizer {name}: z {tuple(z.shape)} max|grad| {float(z.grad.abs().max()):.3f}")
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
