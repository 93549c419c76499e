#!/usr/bin/env python3
"""Generate tests/golden/stft_loss.npz: known answers of the reference's multi-resolution STFT loss (losses/stft_loss.py) and
waveform-shape loss (losses/waveform_loss.py).

Runs only where the reference is available.  It imports the UNMODIFIED reference modules ``losses.stft_loss`` and
``losses.waveform_loss``; the ``losses`` package pulls in librosa, so the import goes through
make_mel_golden.import_mel_loss(), which handles a missing librosa.

From the reference on the CPU in float32 it stores, for every parameter set of stft_oracle.PARAMS and input of
stft_oracle.INPUTS, the two losses (``<p>_<i>_sc``, ``<p>_<i>_mag``); for stft_oracle.MAG_CASES the magnitudes of y per
resolution (``<p>_<i>_ymag<r>``, (n, frames, bins)); for every window list of stft_oracle.SHAPE_WINLENS and input of
stft_oracle.SHAPE_INPUTS the shape loss (``shape_<w>_<i>``).  Inputs are regenerated from seeds (stft_oracle.inputs), not
stored.  Fixed member times: a rerun on the same software gives the same bytes.
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

import stft_oracle as SO  # noqa: E402
from make_mel_golden import import_mel_loss  # noqa: E402

OUT = os.path.join(HERE, "stft_loss.npz")


def main():
    import_mel_loss()                                   # puts the reference on sys.path, with librosa or its stand-in
    from losses import stft_loss, waveform_loss
    torch.set_num_threads(4)
    out = {}
    with torch.no_grad():
        for pname, p in SO.PARAMS.items():
            loss = stft_loss.MultiResolutionSTFTLoss(**p)
            for iname in SO.INPUTS:
                x, y = (torch.from_numpy(a) for a in SO.inputs(pname, iname))
                sc, mag = loss(x, y)
                out[f"{pname}_{iname}_sc"] = np.float32(sc)
                out[f"{pname}_{iname}_mag"] = np.float32(mag)
                if (pname, iname) in SO.MAG_CASES:
                    y2 = y.reshape(-1, y.shape[-1])
                    for r, f in enumerate(loss.stft_losses):
                        out[f"{pname}_{iname}_ymag{r}"] = stft_loss.stft(y2, f.fft_size, f.hop_size, f.win_length,
                                                                          f.window).numpy().astype(np.float32)
                print(f"{pname} {iname}: sc {float(sc):.7g} mag {float(mag):.7g}")
        for wname in SO.SHAPE_WINLENS:
            for iname in SO.SHAPE_INPUTS:
                y_hat, y = (torch.from_numpy(a) for a in SO.inputs("defaults", iname))
                y_hat, y = y_hat.reshape(-1, 1, y_hat.shape[-1]), y.reshape(-1, 1, y.shape[-1])
                loss = waveform_loss.MultiWindowShapeLoss(SO.shape_winlens(wname, y.shape[-1]))
                out[f"shape_{wname}_{iname}"] = np.float32(loss(y_hat, y))
                print(f"shape {wname} {iname}: {float(out[f'shape_{wname}_{iname}']):.7g}")
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
