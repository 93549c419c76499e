#!/usr/bin/env python3
"""Generate tests/golden/mel_grad.npz: the reference's mel-spectrogram loss (losses/mel_loss.py) run backward by autograd.

Runs only where the reference is available.  It imports the UNMODIFIED reference module ``losses.mel_loss`` the way
make_mel_golden.py does (its librosa stub included) and runs it on the CPU, once in float32 and once in float64 (the module
converted with ``.double()``: the float32 window and filter bank widened, as in mel_grad_oracle).  Per case ``K`` of
mel_grad_oracle.CASES (``K = mel_grad_oracle.key(params, shape)``) and resolution ``r`` it stores
  K_relerr32_vjp<r>   ||vjp32 - vjp64|| / ||vjp64||: MelSpectrogram.forward's VJP of mel_grad_oracle.upstream(...) w.r.t. x = y_hat
  K_relerr32_loss     the same for the gradient of MultiMelSpectrogramLoss(y_hat, y) w.r.t. y_hat
  K_signdiff          elements (all resolutions) where sign(logmel(y_hat) - logmel(y)) differs between the two runs
  K_vjp<r>, K_lossgrad   the float32 gradients themselves, for cases of at most mel_grad_oracle.STORE_MAX_SAMPLES samples
Inputs are regenerated from seeds, not stored.  Fixed member times: a rerun on the same software gives the same bytes.
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

import mel_grad_oracle as GO  # noqa: E402
from make_mel_golden import import_mel_loss  # noqa: E402

OUT = os.path.join(HERE, "mel_grad.npz")


def run(loss, y_hat, y, ups, dtype):
    """(per-resolution VJPs, loss gradient, per-resolution signs) of the reference module `loss` in `dtype`."""
    b = torch.from_numpy(y).to(dtype)
    vjps, signs = [], []
    for f, g in zip(loss.mel_transfers, ups):
        a = torch.from_numpy(y_hat).to(dtype).requires_grad_(True)
        lm = f(a)
        lm.backward(torch.from_numpy(g).to(dtype))
        vjps.append(a.grad.reshape(-1, a.shape[-1]).numpy().copy())
        with torch.no_grad():
            signs.append(torch.sign(lm.detach() - f(b)).numpy())
    a = torch.from_numpy(y_hat).to(dtype).requires_grad_(True)
    loss(a, b).backward()
    return vjps, a.grad.reshape(-1, a.shape[-1]).numpy().copy(), signs


def main():
    mel_loss, source = import_mel_loss()
    torch.set_num_threads(4)
    out = {"melmat_source": np.asarray(source)}
    for pname, shape in GO.CASES:
        p = GO.params(pname)
        K = GO.key(pname, shape)
        y_hat, y = GO.inputs(shape)
        ups = [GO.upstream(pname, shape, r, p) for r in range(len(p["fft_sizes"]))]
        l32 = mel_loss.MultiMelSpectrogramLoss(**p)
        l64 = mel_loss.MultiMelSpectrogramLoss(**p).double()
        v32, g32, s32 = run(l32, y_hat, y, ups, torch.float32)
        v64, g64, s64 = run(l64, y_hat, y, ups, torch.float64)
        for r in range(len(ups)):
            out[f"{K}_relerr32_vjp{r}"] = np.float64(GO.rel_l2(v32[r], v64[r]))
            if GO.stored(shape):
                out[f"{K}_vjp{r}"] = v32[r].astype(np.float32)
        out[f"{K}_relerr32_loss"] = np.float64(GO.rel_l2(g32, g64))
        out[f"{K}_signdiff"] = np.int64(sum(int((a != b).sum()) for a, b in zip(s32, s64)))
        if GO.stored(shape):
            out[f"{K}_lossgrad"] = g32.astype(np.float32)
        print(f"{K}: relerr32 vjp {[float(out[f'{K}_relerr32_vjp{r}']) for r in range(len(ups))]} "
              f"loss {float(out[f'{K}_relerr32_loss']):.3g} signdiff {int(out[f'{K}_signdiff'])} "
              f"exact-zero grads {int((g32 == 0).sum())}", flush=True)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{OUT}: {os.path.getsize(OUT)} B ({source})")


if __name__ == "__main__":
    main()
