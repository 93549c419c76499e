#!/usr/bin/env python3
"""Generate tests/golden/univ_disc.npz: known answers of the reference's UnivNet discriminator and GAN losses.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules ``models.vocoder.UnivNet``
(Discriminator), ``losses.adversarial_loss`` and ``losses.feat_match_loss`` the way make_disc_golden.py does.

The reference calls one external function, ``torchaudio.functional.spectrogram`` (discriminator.py:23, 557-566).  Where
torchaudio can be imported the real one is used.  Where it cannot, ``spectrogram_standin`` below is put in its place: written
from torchaudio's documented semantics on top of torch.stft (constant pad on both sides, center=True with reflect padding,
one-sided, abs() for power=1.0).  The fixture's ``torchaudio_real`` says which one made it.  The stand-in lives only here.

Weights and inputs are never stored: both sides regenerate them (univ_disc_oracle.state_dict / inputs).  For every case the
reference runs on the CPU in float32, once on y_hat and once on y; stored per case:
  full cases   ``<case>_d<d>_l<l>``: every feature map of cat([y_hat, y]); ``<case>_spec<i>``: the spectrogram (transposed, as
               the convs see it) of each resolution
  the v3 case  ``v3_d<d>_final``, ``v3_d<d>_l<l>_stats`` / ``_sample`` / ``_shape`` as disc.npz's v1 case, and
               ``v3_spec<i>_sample`` / ``_shape``
  every case   ``<case>_gen`` / ``<case>_dis`` / ``<case>_fm``: the losses under disc_oracle's flag lists
  per params   ``keys_<params>``: the reference's state-dict keys in its order
and ``t_min_rejected``: the length below T_MIN that the reference was seen to reject.  Fixed member times.
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

import univ_disc_oracle as UO  # noqa: E402

OUT = os.path.join(HERE, "univ_disc.npz")


def spectrogram_standin(waveform, pad, window, n_fft, hop_length, win_length, power, normalized, center=True,
                        pad_mode="reflect", onesided=True, return_complex=None):
    """torchaudio.functional.spectrogram for the arguments the reference passes (power=1.0, normalized=False)."""
    assert power == 1.0 and normalized is False
    if pad > 0:
        waveform = torch.nn.functional.pad(waveform, (pad, pad), "constant")
    shape = waveform.size()
    waveform = waveform.reshape(-1, shape[-1])
    spec = torch.stft(input=waveform, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center,
                      pad_mode=pad_mode, normalized=False, onesided=onesided, return_complex=True)
    spec = spec.reshape(shape[:-1] + spec.shape[-2:])
    return spec.abs()


def import_reference():
    real = True
    try:
        import torchaudio.functional  # noqa: F401
    except ImportError:
        real = False
        ta = types.ModuleType("torchaudio")
        ta.functional = types.ModuleType("torchaudio.functional")
        ta.functional.spectrogram = spectrogram_standin
        sys.modules["torchaudio"] = ta
        sys.modules["torchaudio.functional"] = ta.functional
    from make_mel_golden import import_mel_loss
    import_mel_loss()                                  # puts the reference on sys.path; librosa stub if needed
    from models.vocoder.UnivNet import Discriminator
    from losses.adversarial_loss import DiscriminatorAdversarialLoss, GeneratorAdversarialLoss
    from losses.feat_match_loss import FeatureMatchLoss
    import models.vocoder.modules.discriminator as M
    return Discriminator, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss, FeatureMatchLoss, M.spectrogram, real


def main():
    Disc, GenAdv, DisAdv, FM, spectrogram, real = import_reference()
    torch.set_num_threads(4)
    out = {"torchaudio_real": np.array([int(real)], np.int64)}
    models = {}
    with torch.no_grad():
        for case, (pname, _) in UO.CASES.items():
            if pname not in models:
                m = Disc(**UO.PARAMS[pname])
                out[f"keys_{pname}"] = np.array(list(m.state_dict().keys()))
                m.load_state_dict(UO.state_dict(pname))            # strict: the window buffers included
                models[pname] = m.eval()
            m = models[pname]
            y_hat, y = UO.inputs(case)
            p_ = m(torch.from_numpy(y_hat))
            p = m(torch.from_numpy(y))
            full_case = case in UO.FULL_CASES
            x = torch.from_numpy(np.concatenate([y_hat, y], 0))
            if x.shape[1] != 1:
                x = x.reshape(-1, 1, x.shape[-1])
            for i, sub in enumerate(m.mrsd.discriminators):
                s = spectrogram(x, pad=sub.win_length // 2, window=sub.window, n_fft=sub.fft_size, hop_length=sub.hop_size,
                                win_length=sub.win_length, power=1.0, normalized=False).transpose(-1, -2)[:, 0]
                s = s.numpy().astype(np.float32)
                if full_case:
                    out[f"{case}_spec{i}"] = s
                else:
                    out[f"{case}_spec{i}_sample"] = s.reshape(-1)[UO.sample_index(s.size)]
                    out[f"{case}_spec{i}_shape"] = np.asarray(s.shape, np.int64)
            for d, (oh, o) in enumerate(zip(p_, p)):
                for l, (th, t) in enumerate(zip(oh, o)):
                    full = torch.cat([th, t], 0).numpy().astype(np.float32)
                    if full_case:
                        out[f"{case}_d{d}_l{l}"] = full
                    else:
                        flat = full.reshape(-1).astype(np.float64)
                        out[f"{case}_d{d}_l{l}_stats"] = np.array([flat.mean(), np.abs(flat).mean()])
                        out[f"{case}_d{d}_l{l}_sample"] = full.reshape(-1)[UO.sample_index(flat.size)]
                        out[f"{case}_d{d}_l{l}_shape"] = np.asarray(full.shape, np.int64)
                        if l == len(o) - 1:
                            out[f"{case}_d{d}_final"] = full
            out[f"{case}_gen"] = np.array([float(GenAdv(average_by_discriminators=a, loss_type=t)(p_)) for a, t in UO.GEN_FLAGS],
                                          np.float32)
            out[f"{case}_dis"] = np.array([[float(v) for v in DisAdv(average_by_discriminators=a, loss_type=t)(p_, p)]
                                           for a, t in UO.DIS_FLAGS], np.float32)
            out[f"{case}_fm"] = np.array([float(FM(average_by_layers=a, average_by_discriminators=b, include_final_outputs=c)(p_, p))
                                          for a, b, c in UO.FM_FLAGS], np.float32)
            print(f"{case}: gen {out[case + '_gen'][0]:.7g} dis {out[case + '_dis'][0]} fm {out[case + '_fm'][0]:.7g}")
        # the shortest accepted length: T_MIN ran above; one sample fewer must be rejected by the reference itself
        try:
            models["short"](torch.zeros(1, 1, UO.T_MIN - 1))
        except RuntimeError as e:
            print(f"T = {UO.T_MIN - 1} rejected by the reference: {str(e).splitlines()[0]}")
            out["t_min_rejected"] = np.array([UO.T_MIN - 1], np.int64)
        else:
            raise SystemExit(f"the reference accepts T = {UO.T_MIN - 1}: T_MIN is wrong")
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
