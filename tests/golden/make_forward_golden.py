#!/usr/bin/env python3
"""Generate tests/golden/forward.npz: known answers of the reference's FULL forward, with the VQ loss and perplexity.

Runs only where the reference is available.  It imports the UNMODIFIED reference the way make_golden.py does, builds its
modules from the seeded synthetic weights (audiodec_amd/synth.py) and runs them in .eval() -- the training-mode
VectorQuantize.forward would update its EMA buffers (layers/vq_module.py:75-81):

  * ``Generator.forward`` (models/autoencoder/AudioDec.py:112-120) -> y, zq, z, vqloss, perplexity, for
      - ``b3``:     vctk_sym, x (3, 1, 4500)
      - ``mono2``:  vctk_sym fed (1, 2, 3000): the mono model's (B, C, T) -> (B', C', T) reshape
      - ``stereo``: test_stereo_sym, x (1, 2, 3000)
    x is synth.synth_audio(SEED, stream, L) for the stored stream ids, reshaped to the stored shape;
  * ``ResidualVQ.forward`` (layers/vq_module.py:119-134) -> losses, perplexities, and forward_index's codes (int16, per stage)
    on latents (1, N, 64), N = 1, 7, 300, 1000, with the codebooks of vctk_sym (8 stages) and of the c16 model (16 stages).
    The latents are numpy.random.default_rng(seed).standard_normal((1, N, 64)) in float32 times the float32 RMS of the
    first stage's codebook (stored), so the tests regenerate them and they are not stored.

Only outputs, seeds and shapes are stored.  The archive is written with fixed member times: a rerun on the same software
gives the same bytes.
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

from audiodec_amd import configs, synth  # noqa: E402
from make_golden import SEED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "forward.npz")

# name: (model alias, shape of x, stream ids of synth.synth_audio, length per stream)
FORWARD = {
    "b3": ("vctk_sym", (3, 1, 4500), [0, 1, 2], 4500),
    "mono2": ("vctk_sym", (1, 2, 3000), [10, 11], 3000),
    "stereo": ("test_stereo_sym", (1, 2, 3000), [20, 21], 3000),
}
# name: (model alias whose codebooks are used, stages)
RVQ = {"sym8": ("vctk_sym", 8), "c16": ("vctk_c16h320_sym", 16)}
RVQ_ROWS = [1, 7, 300, 1000]


def forward_input(shape, streams, length):
    """The input of a forward case: what the tests rebuild."""
    return np.stack([synth.synth_audio(SEED, s, length) for s in streams]).astype(np.float32).reshape(shape)


def codebook_rms(embed0):
    return np.float32(np.sqrt(np.mean(np.square(embed0.astype(np.float64)))))


def rvq_latents(seed, n, rms):
    return np.random.default_rng(seed).standard_normal((1, n, 64)).astype(np.float32) * np.float32(rms)


def rvq_seed(name, n):
    return 1000 * (1 + list(RVQ).index(name)) + n


def main():
    import_reference()
    from models.autoencoder.AudioDec import Generator
    from layers.vq_module import ResidualVQ
    torch.set_num_threads(4)
    out = {"seed": np.int64(SEED)}
    with torch.no_grad():
        for name, (model, shape, streams, length) in FORWARD.items():
            _, enc_tag, _, _, _ = configs.alias(model)
            _, _, pe = configs.experiment(enc_tag)
            g = Generator(**pe)
            g.load_state_dict(synth.synth_state_dict(enc_tag, SEED))
            g.eval()
            x = torch.from_numpy(forward_input(shape, streams, length))
            y, zq, z, vqloss, ppl = g(x)
            out[f"{name}_shape"] = np.asarray(shape, np.int64)
            out[f"{name}_streams"] = np.asarray(streams, np.int64)
            for k, v in (("y", y), ("zq", zq), ("z", z), ("vqloss", vqloss), ("perplexity", ppl)):
                out[f"{name}_{k}"] = v.numpy().astype(np.float32)
            print(f"forward {name}: y {tuple(y.shape)} vqloss {vqloss.numpy()} perplexity {ppl.numpy()}")
        for name, (model, n_q) in RVQ.items():
            _, enc_tag, _, _, _ = configs.alias(model)
            sd = synth.synth_state_dict(enc_tag, SEED)
            pre = "quantizer.codebook."
            rvq = ResidualVQ(num_quantizers=n_q, dim=64, codebook_size=1024)
            rvq.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
            rvq.eval()
            rms = codebook_rms(sd[pre + "layers.0.embed"].numpy())
            out[f"rvq_{name}_rms"] = rms
            for n in RVQ_ROWS:
                x = torch.from_numpy(rvq_latents(rvq_seed(name, n), n, rms))
                _, losses, ppls = rvq(x)
                _, codes = rvq.forward_index(x)
                out[f"rvq_{name}_{n}_losses"] = losses.numpy().astype(np.float32)
                out[f"rvq_{name}_{n}_perplexities"] = ppls.numpy().astype(np.float32)
                out[f"rvq_{name}_{n}_codes"] = codes.reshape(n_q, n).numpy().astype(np.int16)
            print(f"ResidualVQ {name}: rows {RVQ_ROWS}, last perplexities {ppls.numpy()}")
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
