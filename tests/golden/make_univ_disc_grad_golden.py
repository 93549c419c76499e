#!/usr/bin/env python3
"""Generate tests/golden/univ_disc_grad.npz: the reference's generator-side GAN loss through the UnivNet discriminator, run
backward to y_hat by autograd.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules the way make_univ_disc_golden.py does
(with that file's ``torchaudio.functional.spectrogram`` stand-in where torchaudio cannot be imported; the fixture's
``torchaudio_real`` says which) and, for every case of univ_disc_grad_oracle.CASES and flag set of disc_grad_oracle.FLAGS, runs the
reference on the CPU in float32 as its generator step does (trainer/autoencoder.py:102-108): D(y) under no_grad, D(y_hat) with the
graph, ``UPSTREAM * lambda_adv * (gen_adv(p_) + lambda_feat_match * feat_match(p_, p))`` backward.  Stored per case ``C`` and flag
set ``F``:
  C_F_grad   the reference's float32 gradient with respect to y_hat
  C_F_eref   max |that - grad64 at the reference's own float32 decisions| (univ_disc_grad_oracle.grad64)
  C_F_gmax   max |grad64 at those decisions|
and per full-map case (every one but v3)
  C_bounds   test_gpu_univnet_discriminator's bound of every layer in (d, l) order, from the reference's float32 feature maps of
             cat([y_hat, y]) and the fp64 ones
  C_flips    the number of decisions (LeakyReLU masks and L1 signs) the reference took differently from fp64.
It ASSERTS 0 < eref <= 1e-5 gmax and, for the full-map cases, that the reference's decisions differ from the fp64 ones only at
elements whose fp64 margin is within that bound.  Weights and inputs are regenerated from seeds, never stored.  Fixed member times:
a rerun on the same software gives the same bytes.
"""
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

import univ_disc_grad_oracle as GO  # noqa: E402
import univ_disc_oracle as UO  # noqa: E402
from make_univ_disc_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "univ_disc_grad.npz")


def main():
    Disc, GenAdv, _, FM, _, real = import_reference()
    torch.set_num_threads(4)
    out, models = {"torchaudio_real": np.array([int(real)], np.int64)}, {}
    for case, (pname, _) in GO.CASES.items():
        if pname not in models:
            m = Disc(**UO.PARAMS[pname])
            m.load_state_dict(UO.state_dict(pname))
            models[pname] = m.eval()
        m, sd = models[pname], UO.state_dict(pname)
        y_hat, y = GO.inputs(case)
        with torch.no_grad():
            p = m(torch.from_numpy(y))
            f64_hat = GO.features64(pname, sd, torch.from_numpy(y_hat).double())
            f64 = GO.features64(pname, sd, torch.from_numpy(y).double())
        masks = signs = None
        for flags, f in GO.FLAGS.items():
            a = torch.from_numpy(y_hat).clone().requires_grad_(True)
            p_ = m(a)
            loss = GenAdv(average_by_discriminators=f["gen"][0], loss_type=f["gen"][1])(p_)
            if f["fm"] is not None:
                fm = FM(average_by_layers=f["fm"][0], average_by_discriminators=f["fm"][1], include_final_outputs=f["fm"][2])
                loss = loss + f["lambda_feat_match"] * fm(p_, p)
            (GO.UPSTREAM * (f["lambda_adv"] * loss)).backward()
            ref = a.grad.numpy().copy()
            if masks is None:
                masks, signs = GO.decisions(p_, p)
                if case in GO.FULL_CASES:
                    cat = lambda h, r: [[np.concatenate([GO._np(u), GO._np(v)], 0) for u, v in zip(oh, o)] for oh, o in zip(h, r)]
                    bounds = GO.layer_bounds(cat(p_, p), cat(f64_hat, f64))
                    m64, s64 = GO.decisions(f64_hat, f64)
                    found, ok = GO.disagreements(masks, signs, m64, s64, GO.margins64(f64_hat, f64), bounds)
                    for d, l, what, n, worst, bound in found:
                        print(f"  {case} d{d} l{l}: {n} {what} decisions differ from fp64, worst margin {worst:.3g}, bound {bound:.3g}")
                    assert ok, f"{case}: a reference decision differs from fp64 outside the forward bound"
                    out[f"{case}_bounds"] = bounds
                    out[f"{case}_flips"] = np.array(sum(n for _, _, _, n, _, _ in found), np.int64)
            exact = GO.grad64(pname, sd, y_hat, y, flags, masks, signs)
            eref, gmax = float(np.max(np.abs(ref - exact))), float(np.max(np.abs(exact)))
            print(f"{case} {flags}: E_ref {eref:.3g}  max|grad64| {gmax:.3g}  ratio {eref / gmax:.3g}")
            assert np.isfinite(ref).all() and 0 < eref <= 1e-5 * gmax, f"{case} {flags}: E_ref {eref:.3g} against max|grad64| {gmax:.3g}"
            out[f"{case}_{flags}_grad"] = ref.astype(np.float32)
            out[f"{case}_{flags}_eref"] = np.array(eref)
            out[f"{case}_{flags}_gmax"] = np.array(gmax)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{OUT}: {os.path.getsize(OUT)} B  (torchaudio_real = {int(real)})")


if __name__ == "__main__":
    main()
