#!/usr/bin/env python3
"""Generate tests/golden/disc_train.npz: the reference's discriminator step run backward to its parameters by autograd.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules the way make_disc_golden.py does and,
for every case of disc_train_oracle.CASES and flag set of disc_train_oracle.FLAGS, runs the reference ``Discriminator`` (train
mode) and ``DiscriminatorAdversarialLoss`` on the CPU in float32 as its discriminator step does (trainer/autoencoder.py:117-126):
``p = D(y)``, ``p_ = D(y_hat)``, ``UPSTREAM * (real_loss + fake_loss)`` backward.  Stored per parameter set ``P`` (reduced, v1):
  P_names, P_shapes   the reference's ``named_parameters()``: names, and shapes padded with zeros to four entries
and per case ``C`` and flag set ``F``, over the parameters in that order:
  C_F_grad   the reference's float32 gradients at disc_train_oracle.param_index of each parameter, concatenated: every entry of
             a parameter of up to N_FULL entries in the reduced-width cases, N_FULL sampled entries of a larger one, N_SAMPLE
             sampled entries in v1 (every entry of every reduced-width case would be 2.7 MB)
  C_F_eref   per parameter, max |reference gradient - grads64 at the reference's own float32 LeakyReLU decisions|, all entries
  C_F_gmax   per parameter, max |grads64 at those decisions|
It ASSERTS, per parameter, ``4 E_ref + 1e-6 gmax <= 5e-5 gmax`` and ``gmax > 0``: the bound the HIP path is held to is a small
fraction of every gradient.  Weights and inputs are regenerated from seeds, never stored.  Fixed member times: a rerun on the
same software gives the same bytes.
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

import disc_oracle as DO  # noqa: E402
import disc_train_oracle as TO  # noqa: E402
from make_disc_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "disc_train.npz")
CAP = 5e-5


def main():
    Disc, _, DisAdv, _ = import_reference()
    torch.set_num_threads(4)
    out, models = {}, {}
    for case, (pname, _) in TO.CASES.items():
        if pname not in models:
            m = Disc(**DO.PARAMS[pname])
            m.load_state_dict(DO.state_dict(pname))
            models[pname] = m.train()
            names = [k for k, _ in m.named_parameters()]
            assert sorted(names) == sorted(DO.state_dict(pname)), "the reference's parameters are not the state dict's keys"
            out[f"{pname}_names"] = np.array(names)
            out[f"{pname}_shapes"] = np.array([list(q.shape) + [0] * (4 - q.dim()) for _, q in m.named_parameters()], np.int64)
        m, sd = models[pname], DO.state_dict(pname)
        names = [k for k, _ in m.named_parameters()]
        full = pname == "reduced"
        y_hat, y = TO.inputs(case)
        for flags in TO.FLAGS:
            m.zero_grad(set_to_none=True)
            p = m(torch.from_numpy(y))
            p_ = m(torch.from_numpy(y_hat))
            real_loss, fake_loss = DisAdv(**TO.loss_params(flags))(p_, p)
            (TO.UPSTREAM * (real_loss + fake_loss)).backward()
            ref = {k: q.grad.detach().numpy().copy() for k, q in m.named_parameters()}
            exact = TO.grads64(pname, sd, y_hat, y, flags, TO.masks_of(p_), TO.masks_of(p))
            eref = np.array([np.max(np.abs(ref[k].astype(np.float64) - exact[k])) for k in names])
            gmax = np.array([np.max(np.abs(exact[k])) for k in names])
            worst = int(np.argmax((4 * eref + 1e-6 * gmax) / gmax))
            print(f"{case} {flags}: worst E_ref / gmax {float(np.max(eref / gmax)):.3g} ({names[worst]}), min gmax {gmax.min():.3g}")
            assert np.all(gmax > 0), f"{case} {flags}: an all-zero gradient: {[k for k, g in zip(names, gmax) if not g > 0]}"
            assert np.all(4 * eref + 1e-6 * gmax <= CAP * gmax), f"{case} {flags}: {names[worst]} is outside the cap"
            out[f"{case}_{flags}_grad"] = np.concatenate([ref[k].reshape(-1)[TO.param_index(ref[k].size, full)] for k in names]).astype(np.float32)
            out[f"{case}_{flags}_eref"], out[f"{case}_{flags}_gmax"] = eref, gmax
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{OUT}: {os.path.getsize(OUT)} B")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
