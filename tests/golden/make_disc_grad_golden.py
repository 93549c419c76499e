#!/usr/bin/env python3
"""Generate tests/golden/disc_grad.npz: the reference's generator-side GAN loss run backward to y_hat by autograd.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules the way make_disc_golden.py does and,
for every case of disc_grad_oracle.CASES and flag set of disc_grad_oracle.FLAGS, runs the reference on the CPU in float32 as its
generator step does (trainer/autoencoder.py:102-108): D(y) under no_grad, D(y_hat) with the graph,
``UPSTREAM * lambda_adv * (gen_adv(p_) + lambda_feat_match * feat_match(p_, p))`` backward.  Stored per case ``C`` and flag set ``F``:
  C_F_grad   the reference's float32 gradient with respect to y_hat
  C_F_eref   max |that - grad64 at the reference's own float32 decisions| (disc_grad_oracle.grad64)
  C_F_gmax   max |grad64 at those decisions|
and per reduced-width case
  C_bounds   test_gpu_discriminator._bound of every layer in (d, l) order, from the reference's float32 feature maps of
             cat([y_hat, y]) and the fp64 ones
  C_flips    the number of decisions (LeakyReLU masks and L1 signs) the reference took differently from fp64.
For the reduced-width cases it also ASSERTS that the reference's decisions differ from the fp64 ones only at elements whose fp64
margin is within that bound.  Weights and inputs are regenerated from seeds, never stored.  Fixed member times: a rerun on the same
software gives the same bytes.
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

import disc_grad_oracle as GO  # noqa: E402
import disc_oracle as DO  # noqa: E402
from make_disc_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "disc_grad.npz")


def main():
    Disc, GenAdv, _, FM = import_reference()
    torch.set_num_threads(4)
    out, models = {}, {}
    for case, (pname, _) in GO.CASES.items():
        if pname not in models:
            m = Disc(**DO.PARAMS[pname])
            m.load_state_dict(DO.state_dict(pname))
            models[pname] = m.eval()
        m, sd = models[pname], DO.state_dict(pname)
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
                if pname == "reduced":
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
            out[f"{case}_{flags}_grad"] = ref.astype(np.float32)
            out[f"{case}_{flags}_eref"] = np.array(np.max(np.abs(ref - exact)))
            out[f"{case}_{flags}_gmax"] = np.array(np.max(np.abs(exact)))
            print(f"{case} {flags}: E_ref {float(out[f'{case}_{flags}_eref']):.3g}  max|grad64| {float(out[f'{case}_{flags}_gmax']):.3g}")
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
