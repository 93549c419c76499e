#!/usr/bin/env python3
"""Time the residual-VQ EMA codebook update (adk_rvq_ema_update) at the shipped quantizer's shape.

Shapes: 8 stages x 1024 codes x 64 components at 512, 4096 and 32768 rows (frames x streams of one training batch / of a second of a
256-stream deployment).  The codes are the search's own (adk_rvq_encode on the table being updated), the latents N(0, 1) times the
first stage's RMS.  Every timed call starts from the same state (the buffers are restored by device copies outside the timed
region).  Device events after 5 warm-up runs, median of 20.  bytes: the residuals written and read once (2 x n_q x rows x dim x 4)
plus the tables read and written (embed, embed_avg, sums, row-major twins: 7 x n_q x size x dim x 4).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from audiodec_amd import codebook_ema  # noqa: E402

N_Q, SIZE, DIM = 8, 1024, 64
ROWS = (512, 4096, 32768)
REPS, WARM = 20, 5


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    embeds = [torch.randn(DIM, SIZE, generator=g) * 0.5 ** s for s in range(N_Q)]
    cs = [torch.rand(SIZE, generator=g) * 4 for _ in range(N_Q)]
    first = codebook_ema.State.from_buffers(embeds, cs, [e * c.clamp(min=0.3) for e, c in zip(embeds, cs)], dev)
    keep = [t.clone() for t in (first.embed, first.enorm, first.codebook, first.cluster_size, first.embed_avg)]
    for n in ROWS:
        z = torch.randn(n, DIM, generator=g).to(dev).contiguous()
        idx = codebook_ema.search(first, z)
        ts = []
        for rep in range(WARM + REPS):
            for t, k in zip((first.embed, first.enorm, first.codebook, first.cluster_size, first.embed_avg), keep):
                t.copy_(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            codebook_ema.update(first, z, idx)
            e1.record()
            e1.synchronize()
            if rep >= WARM:
                ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        us = ts[len(ts) // 2]
        mb = (2 * N_Q * n * DIM * 4 + 7 * N_Q * SIZE * DIM * 4) / 1e6
        print(json.dumps(dict(op="rvq_ema_update", n_q=N_Q, size=SIZE, dim=DIM, rows=n, us=round(us, 1), min_us=round(ts[0], 1),
                              max_us=round(ts[-1], 1), reps=REPS, mbytes=round(mb, 1), gbytes_per_s=round(mb / 1e3 / (us * 1e-6), 1))),
              flush=True)
        for t, k in zip((first.embed, first.enorm, first.codebook, first.cluster_size, first.embed_avg), keep):
            t.copy_(k)


if __name__ == "__main__":
    main()
