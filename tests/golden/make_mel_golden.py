#!/usr/bin/env python3
"""Generate tests/golden/mel.npz: known answers of the reference's mel-spectrogram loss (losses/mel_loss.py).

Runs only where the reference is available.  It imports the UNMODIFIED reference module ``losses.mel_loss`` the way
make_golden.py imports the reference.  That module imports librosa for ``librosa.filters.mel``; when librosa cannot be
imported, a stub module is injected whose ``filters.mel`` is an independent NumPy restatement of librosa's defaults (Slaney
mel scale, Slaney norm, float32 output).  Which one was used is recorded as ``melmat_source``.

For every parameter set of mel_oracle.PARAMS and input of mel_oracle.INPUTS it stores, from the reference on the CPU in
float32: the melmat of each resolution (``<p>_melmat<r>``, librosa layout (n_mels, bins)), the loss
(``<p>_<i>_loss``) and, for mel_oracle.LOGMEL_CASES, the log-mels of y per resolution (``<p>_<i>_logmel<r>``).  Also
``b3_loss``: vctk params, the reference's own Generator output y of forward.npz case b3 against its input x.  Inputs are
regenerated from seeds (mel_oracle.inputs), not stored.  Fixed member times: a rerun on the same software gives the same bytes.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import mel_oracle as MO  # noqa: E402
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, "mel.npz")


def _stub_mel(*, sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, norm="slaney", dtype=np.float32):
    """librosa.filters.mel with its defaults, restated from the Slaney definition."""
    assert not htk and norm == "slaney"
    if fmax is None:
        fmax = float(sr) / 2
    lin, brk, brk_mel, step = 200.0 / 3, 1000.0, 15.0, np.log(6.4) / 27.0

    def to_mel(f):
        f = np.atleast_1d(np.asarray(f, np.float64))
        m = f / lin
        hi = f >= brk
        m[hi] = brk_mel + np.log(f[hi] / brk) / step
        return m

    def to_hz(m):
        m = np.asarray(m, np.float64)
        f = lin * m
        hi = m >= brk_mel
        f[hi] = brk * np.exp(step * (m[hi] - brk_mel))
        return f

    out = np.zeros((n_mels, 1 + n_fft // 2), dtype=dtype)
    bins_hz = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    edges = to_hz(np.linspace(to_mel(fmin)[0], to_mel(fmax)[0], n_mels + 2))
    width = np.diff(edges)
    for m in range(n_mels):
        rise = (bins_hz - edges[m]) / width[m]
        fall = (edges[m + 2] - bins_hz) / width[m + 1]
        out[m] = np.maximum(0, np.minimum(rise, fall))
    out *= (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[:, None]
    return out


def import_mel_loss():
    try:
        import librosa  # noqa: F401
        source = "librosa " + librosa.__version__
    except ImportError:
        lb = types.ModuleType("librosa")
        lb.filters = types.ModuleType("librosa.filters")
        lb.filters.mel = _stub_mel
        sys.modules["librosa"] = lb
        sys.modules["librosa.filters"] = lb.filters
        source = "numpy restatement of librosa.filters.mel (librosa not importable)"
    if REF not in sys.path:
        sys.path.insert(1, REF)
    from losses import mel_loss
    return mel_loss, source


def main():
    mel_loss, source = import_mel_loss()
    torch.set_num_threads(4)
    out = {"melmat_source": np.asarray(source)}
    with torch.no_grad():
        for pname in MO.PARAMS:
            p = MO.params(pname)
            kw = {k: v for k, v in p.items()}
            loss = mel_loss.MultiMelSpectrogramLoss(**kw)
            for r, f in enumerate(loss.mel_transfers):
                out[f"{pname}_melmat{r}"] = f.melmat.numpy().T.astype(np.float32)
            for iname in MO.INPUTS:
                y_hat, y = MO.inputs(pname, iname)
                v = loss(torch.from_numpy(y_hat), torch.from_numpy(y))
                out[f"{pname}_{iname}_loss"] = np.float32(v)
                if (pname, iname) in MO.LOGMEL_CASES:
                    for r, f in enumerate(loss.mel_transfers):
                        out[f"{pname}_{iname}_logmel{r}"] = f(torch.from_numpy(y)).numpy().astype(np.float32)
                print(f"{pname} {iname}: loss {float(v):.7g}")
        fw = np.load(os.path.join(HERE, "forward.npz"), allow_pickle=False)
        import make_forward_golden as MFG
        shape, streams = tuple(fw["b3_shape"]), list(fw["b3_streams"])
        x = MFG.forward_input(shape, streams, shape[-1])
        loss = mel_loss.MultiMelSpectrogramLoss(**MO.params("vctk"))
        out["b3_loss"] = np.float32(loss(torch.from_numpy(fw["b3_y"]), torch.from_numpy(x)))
        print(f"b3: loss {float(out['b3_loss']):.7g}")
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
