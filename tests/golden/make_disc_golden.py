#!/usr/bin/env python3
"""Generate tests/golden/disc.npz: known answers of the reference's HiFi-GAN discriminator and GAN losses.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules ``models.vocoder.HiFiGAN``
(Discriminator), ``losses.adversarial_loss`` and ``losses.feat_match_loss`` the way make_golden.py imports the reference.
torchaudio is imported there only for UnivNet's spectrogram (discriminator.py:23); it is stubbed in sys.modules when absent.
The ``losses`` package also imports librosa (for mel_loss, not used here); make_mel_golden.import_mel_loss stubs it the same way.

Weights are never stored: both sides regenerate them with synth.discriminator_state_dict(params, disc_oracle.SEED).  Inputs
are regenerated from seeds too (disc_oracle.inputs).  For every case of disc_oracle.CASES the reference runs on the CPU in
float32, as its eval step does, once on y_hat and once on y (trainer/autoencoder.py:158-163); stored per case:
  reduced-width cases  ``<case>_d<d>_l<l>``: every feature map of cat([y_hat, y]) (the two runs concatenated on the batch)
  the v1 case          ``v1_d<d>_final``: final outputs; ``v1_d<d>_l<l>_stats``: (mean, mean |x|) of each feature map;
                       ``v1_d<d>_l<l>_sample``: the entries at disc_oracle.sample_index(size) of each feature map
  every case           ``<case>_gen`` / ``<case>_dis`` / ``<case>_fm``: the losses under disc_oracle.GEN_FLAGS / DIS_FLAGS /
                       FM_FLAGS, from the reference's loss modules.
Fixed member times: a rerun on the same software gives the same bytes.
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

import disc_oracle as DO  # noqa: E402
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, "disc.npz")


def import_reference():
    try:
        import torchaudio  # noqa: F401
    except ImportError:
        ta = types.ModuleType("torchaudio")
        ta.functional = types.ModuleType("torchaudio.functional")
        ta.functional.spectrogram = None
        sys.modules["torchaudio"] = ta
        sys.modules["torchaudio.functional"] = ta.functional
    from make_mel_golden import import_mel_loss
    import_mel_loss()                                  # puts REF on sys.path; librosa stub if needed
    from models.vocoder.HiFiGAN import Discriminator
    from losses.adversarial_loss import DiscriminatorAdversarialLoss, GeneratorAdversarialLoss
    from losses.feat_match_loss import FeatureMatchLoss
    return Discriminator, GeneratorAdversarialLoss, DiscriminatorAdversarialLoss, FeatureMatchLoss


def main():
    Disc, GenAdv, DisAdv, FM = import_reference()
    torch.set_num_threads(4)
    out = {}
    models = {}
    with torch.no_grad():
        for case, (pname, _) in DO.CASES.items():
            if pname not in models:
                m = Disc(**DO.PARAMS[pname])
                m.load_state_dict(DO.state_dict(pname))
                models[pname] = m.eval()
            m = models[pname]
            y_hat, y = DO.inputs(case)
            p_ = m(torch.from_numpy(y_hat))
            p = m(torch.from_numpy(y))
            for d, (oh, o) in enumerate(zip(p_, p)):
                for l, (th, t) in enumerate(zip(oh, o)):
                    full = torch.cat([th, t], 0).numpy().astype(np.float32)
                    if case in DO.FULL_CASES:
                        out[f"{case}_d{d}_l{l}"] = full
                    else:
                        flat = full.reshape(-1).astype(np.float64)
                        out[f"{case}_d{d}_l{l}_stats"] = np.array([flat.mean(), np.abs(flat).mean()])
                        out[f"{case}_d{d}_l{l}_sample"] = full.reshape(-1)[DO.sample_index(flat.size)]
                        out[f"{case}_d{d}_l{l}_shape"] = np.asarray(full.shape, np.int64)
                        if l == len(o) - 1:
                            out[f"{case}_d{d}_final"] = full
            out[f"{case}_gen"] = np.array([float(GenAdv(average_by_discriminators=a, loss_type=t)(p_)) for a, t in DO.GEN_FLAGS],
                                          np.float32)
            out[f"{case}_dis"] = np.array([[float(v) for v in DisAdv(average_by_discriminators=a, loss_type=t)(p_, p)]
                                           for a, t in DO.DIS_FLAGS], np.float32)
            out[f"{case}_fm"] = np.array([float(FM(average_by_layers=a, average_by_discriminators=b, include_final_outputs=c)(p_, p))
                                          for a, b, c in DO.FM_FLAGS], np.float32)
            print(f"{case}: gen {out[case + '_gen'][0]:.7g} dis {out[case + '_dis'][0]} fm {out[case + '_fm'][0]:.7g}")
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
