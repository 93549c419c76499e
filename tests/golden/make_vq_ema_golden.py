#!/usr/bin/env python3
"""Generate tests/golden/vq_ema.npz and vq_ema_c16.npz: known answers of the reference's TRAINING-mode ResidualVQ.forward (the EMA codebook update).

Runs only where the reference is available.  It imports the UNMODIFIED reference the way make_golden.py does, loads a seeded
state into ``ResidualVQ`` (layers/vq_module.py:107-134), and runs ONE forward in ``.train()`` per case:

  case  n_q  dim  size   rows
  c1      3   64   128      1
  c2      3   64   128    300
  c3      8   64  1024   1000
  c4     16   64  1024    257

Initial state (``initial_state``): embed N(0,1) * 0.5^s; cluster_size uniform in [0, 4) with every 7th entry 0 (dead codes);
embed_avg = embed * max(cluster_size, 0.3).  Latents (``latents``): N(0,1) float32.  Both are regenerated from the seeds by the
tests and not stored.  Stored per case: the reference's codes (int16), cluster_size', the losses and perplexities (the eval-mode
values: the training forward computes them against the old table, checked here against an eval-mode copy), embed_avg' and embed'
-- in full for the size-128 cases, every 16th code column for the size-1024 cases.

Only outputs and seeds are stored.  float32 noise does not compress, and the four cases together exceed the 1 MiB a committed file
may have, so the 16-stage case lives in an archive of its own (``archive_of``); ``load`` gives the tests one mapping over both.
The archives are written with fixed member times: a rerun on the same software gives the same bytes.
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

OUT = os.path.join(HERE, "vq_ema.npz")
OUT_C16 = os.path.join(HERE, "vq_ema_c16.npz")
DECAY, EPS = 0.8, 1e-5          # VectorQuantize's defaults (vq_module.py:26-28)

# name: (n_q, dim, size, rows)
CASES = {"c1": (3, 64, 128, 1), "c2": (3, 64, 128, 300), "c3": (8, 64, 1024, 1000), "c4": (16, 64, 1024, 257)}


def archive_of(key):
    return OUT_C16 if key.startswith("c4_") else OUT


def load(golden_dir=HERE):
    """Every stored array of both archives, by key."""
    out = {}
    for path in (OUT, OUT_C16):
        with np.load(os.path.join(golden_dir, os.path.basename(path)), allow_pickle=False) as f:
            out.update({k: f[k] for k in f.files})
    return out


def case_seed(name):
    return 7000 + list(CASES).index(name)


def column_step(size):
    """Stored code columns of embed_avg' / embed': all of a small codebook, every 16th of a large one."""
    return 1 if size <= 128 else 16


def initial_state(seed, n_q, dim, size):
    """(embed (n_q, dim, size), cluster_size (n_q, size), embed_avg (n_q, dim, size)), float32."""
    rng = np.random.default_rng(seed)
    embed = np.stack([(rng.standard_normal((dim, size)) * 0.5 ** s).astype(np.float32) for s in range(n_q)])
    cs = (rng.random((n_q, size)) * 4.0).astype(np.float32)
    cs[:, ::7] = 0.0
    ea = (embed * np.maximum(cs, np.float32(0.3))[:, None, :]).astype(np.float32)
    return embed, cs, ea


def latents(seed, n, dim):
    return np.random.default_rng(seed + 500).standard_normal((n, dim)).astype(np.float32)


def main():
    from make_golden import import_reference
    import_reference()
    from layers.vq_module import ResidualVQ
    torch.set_num_threads(4)
    out = {"decay": np.float64(DECAY), "eps": np.float64(EPS)}
    with torch.no_grad():
        for name, (n_q, dim, size, n) in CASES.items():
            seed = case_seed(name)
            embed, cs, ea = initial_state(seed, n_q, dim, size)
            rvq = ResidualVQ(num_quantizers=n_q, dim=dim, codebook_size=size, decay=DECAY, eps=EPS)
            sd = {}
            for s in range(n_q):
                sd[f"layers.{s}.embed"] = torch.from_numpy(embed[s])
                sd[f"layers.{s}.cluster_size"] = torch.from_numpy(cs[s])
                sd[f"layers.{s}.embed_avg"] = torch.from_numpy(ea[s])
            rvq.load_state_dict(sd)
            x = torch.from_numpy(latents(seed, n, dim))[None]
            ev = copy.deepcopy(rvq).eval()
            _, ev_losses, ev_ppls = ev(x)
            _, codes = ev.forward_index(x)
            rvq.train()
            _, losses, ppls = rvq(x)
            assert torch.equal(losses, ev_losses) and torch.equal(ppls, ev_ppls)
            step = column_step(size)
            new = rvq.state_dict()
            out[f"{name}_seed"] = np.int64(seed)
            out[f"{name}_codes"] = codes.reshape(n_q, n).numpy().astype(np.int16)
            out[f"{name}_losses"] = ev_losses.numpy().astype(np.float32)
            out[f"{name}_perplexities"] = ev_ppls.numpy().astype(np.float32)
            out[f"{name}_cluster_size"] = np.stack([new[f"layers.{s}.cluster_size"].numpy() for s in range(n_q)])
            out[f"{name}_embed_avg"] = np.stack([new[f"layers.{s}.embed_avg"].numpy()[:, ::step] for s in range(n_q)])
            out[f"{name}_embed"] = np.stack([new[f"layers.{s}.embed"].numpy()[:, ::step] for s in range(n_q)])
            print(f"{name}: rows {n}, perplexities {ppls.numpy()[:3]} ...")
    for path in (OUT, OUT_C16):
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
            for k in sorted(out):
                if archive_of(k) != path:
                    continue
                buf = io.BytesIO()
                np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
                info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                zf.writestr(info, buf.getvalue())
        print(f"{path}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
