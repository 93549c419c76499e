"""Residual-VQ statistics on the device: commitment loss, perplexity and code usage (adk_rvq_stats).

The reference reports them from ``ResidualVQ.forward`` (layers/vq_module.py:61-88, 119-134): per stage the loss
``mse(q_s, r_s)`` and the perplexity ``exp(-sum_k p_k log(p_k + 1e-10))`` of the code histogram; its trainers log them per
stage (trainer/autoencoder.py:145-151, trainer/trainerGAN.py:377-401).  Here they come from the codes the search emitted:
``adk_rvq_stats`` rebuilds each row's residual chain with the search's own f32 step and folds the squared errors, the row
count and the histogram into an accumulator that stays on the device.

``fold`` is the one call every user goes through (``layers.ResidualVQ.forward``,
``AutoEncoderStreamGenerator.quantizer_forward(return_stats=True)``, ``CodebookUsage``).  ``CodebookUsage`` keeps one
accumulator across calls -- what a serving deployment needs to see dead codes or a collapsed stage
(``BatchedAudioDecStreamer(track_codebook_usage=True)``).
"""
import ctypes as C

import torch

from . import lazy_guard, native


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def accumulator(n_q, size, device):
    """A zeroed accumulator of adk_rvq_stats on `device`: (counts int64[n_q*size], sse float64[n_q], rows int64[1])."""
    return (torch.zeros(n_q * size, dtype=torch.int64, device=device), torch.zeros(n_q, dtype=torch.float64, device=device),
            torch.zeros(1, dtype=torch.int64, device=device))


def fold(acc, z, codebook, idx, n_q, dim, size, vqloss=None, perplexity=None):
    """adk_rvq_stats on the current stream of the accumulator's device.  z (n_rows, dim) float32 and idx (n_q, n_rows) int64 (the
    emitted indices, stage offset included), both contiguous; z = idx = None folds nothing.  codebook (n_q*size, dim) row-major.
    vqloss / perplexity: float32 (n_q,) tensors to write from the totals after the fold, or None.  Does not synchronise."""
    counts, sse, rows = acc
    dev = sse.device
    n_rows = int(z.shape[0]) if z is not None else 0
    lib = native.lib()
    ws_bytes = int(lib.adk_rvq_stats_workspace_bytes(n_rows, n_q))
    if ws_bytes < 0:
        native.check(ws_bytes, "adk_rvq_stats_workspace_bytes")
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev) if ws_bytes else None
    native.check(lib.adk_rvq_stats(
        _ptr(z), _ptr(codebook), _ptr(idx), n_rows, n_q, dim, size, _ptr(counts), _ptr(sse), _ptr(rows), _ptr(ws),
        _ptr(vqloss), _ptr(perplexity), native.current_stream(dev)), "adk_rvq_stats")


def row_major_codebook(embeds, device):
    """The reference's `embed` buffers, each (dim, size), as one (n_q*size, dim) row-major table (ResidualVQ.initial's layout)."""
    cb = torch.stack([e.detach().float().cpu().transpose(0, 1) for e in embeds])
    return cb.reshape(-1, cb.size(-1)).contiguous().to(device)


class CodebookUsage:
    """Code usage of an ``AutoEncoderStreamGenerator``'s quantizer, accumulated on its device over any number of calls.

    ``update(z, idx)`` folds the latents ``z`` (B, code_dim, T) -- what ``encode`` returned -- and the indices ``idx`` (n_q, B, T)
    or (n_q, T) -- what ``quantize`` returned for them -- into the totals without synchronising.  Results of guarded direct calls
    are verified first (their call log is settled), so an index a guard repair rewrites is counted once, as repaired.
    ``counts()``, ``perplexity()``, ``vqloss()``, ``dead_codes()`` and ``rows()`` read the totals (these synchronise);
    ``reset()`` zeroes them."""

    def __init__(self, generator):
        g = generator
        self.n_q, self.dim, self.size = g.n_q, g.dim, g.size
        self.device = g._dev()
        sd = g._sd
        if sd is None:
            raise native.NativeError("CodebookUsage: the generator has no weights (load_state_dict first)")
        self.codebook = row_major_codebook([sd[f"quantizer.codebook.layers.{i}.embed"] for i in range(self.n_q)], self.device)
        self._acc = accumulator(self.n_q, self.size, self.device)

    def reset(self):
        for t in self._acc:
            t.zero_()
        return self

    def update(self, z, idx):
        z, idx = lazy_guard.settled(z), lazy_guard.settled(idx)
        if z.dim() != 3 or z.shape[1] != self.dim:
            raise ValueError(f"update: z must be (B, {self.dim}, T), got {tuple(z.shape)}")
        B, D, T = z.shape
        idx = idx.to(device=self.device, dtype=torch.int64)
        if idx.dim() == 2:
            idx = idx.unsqueeze(1)
        if tuple(idx.shape) != (self.n_q, B, T):
            raise ValueError(f"update: idx must be ({self.n_q}, {B}, {T}) for z {tuple(z.shape)}, got {tuple(idx.shape)}")
        if B * T == 0:
            return self
        zt = z.to(device=self.device, dtype=torch.float32).transpose(2, 1).reshape(B * T, D).contiguous()
        fold(self._acc, zt, self.codebook, idx.reshape(self.n_q, B * T).contiguous(), self.n_q, self.dim, self.size)
        return self

    def _finalize(self):
        vq = torch.empty(self.n_q, dtype=torch.float32, device=self.device)
        ppl = torch.empty(self.n_q, dtype=torch.float32, device=self.device)
        fold(self._acc, None, None, None, self.n_q, self.dim, self.size, vq, ppl)
        return vq, ppl

    def rows(self):
        """Rows (frames x streams) folded so far."""
        return int(self._acc[2].item())

    def counts(self):
        """(n_q, size) int64: how often each code of each stage was emitted."""
        return self._acc[0].view(self.n_q, self.size).cpu()

    def perplexity(self):
        """(n_q,) float32: exp(-sum_k p_k log(p_k + 1e-10)) of each stage's histogram (NaN before the first row)."""
        return self._finalize()[1].cpu()

    def vqloss(self):
        """(n_q,) float32: mean of (q_s - r_s)^2 over every folded row and component (NaN before the first row)."""
        return self._finalize()[0].cpu()

    def dead_codes(self):
        """(n_q,) int64: codes of each stage never emitted."""
        return (self.counts() == 0).sum(1)
