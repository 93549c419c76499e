"""Residual-VQ codebook re-estimation on the device: the training-mode forward of the quantizer (adk_rvq_ema_update).

``VectorQuantize.forward`` with ``self.training`` set (layers/vq_module.py:74-80) re-estimates each stage's codebook from the batch
it just quantised: the code counts and the per-code sums of the residual rows are folded into ``cluster_size`` / ``embed_avg`` with
an exponential moving average, the cluster sizes are Laplace-smoothed, and ``embed = embed_avg / smoothed``.  It is the one part of
the reference's training that needs no gradient.  ``adk_rvq_ema_update`` does it for all stages of one ``ResidualVQ.forward`` in one
call: the residual chain is rebuilt from the OLD codes with the search's own f32 step, the per-code sums are f64 in ascending row
order (bitwise reproducible, no float atomics), and ``enorm`` and the row-major lookup table are rewritten so that the search and
the lookup can follow on the same stream.

``update(state, z, idx, decay, eps)`` is the one call every user goes through (``layers.ResidualVQ`` in ``train()`` mode,
``CodebookEMA``).  ``CodebookEMA`` adapts the codebook of an ``AutoEncoderStreamGenerator`` to the latents a deployment is already
encoding, continues the reference's statistics exactly as its trainer would have, and saves the result under the reference's
checkpoint keys.
"""
import ctypes as C
import weakref

import torch

from . import codebook_usage, lazy_guard, native


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class State:
    """Device tensors of a residual VQ's codebook and its EMA statistics, all float32 and contiguous:
    embed (n_q, dim, size), enorm (n_q, size), codebook (n_q*size, dim) or None, cluster_size (n_q, size), embed_avg (n_q, dim, size)."""

    def __init__(self, embed, enorm, codebook, cluster_size, embed_avg):
        self.embed, self.enorm, self.codebook, self.cluster_size, self.embed_avg = embed, enorm, codebook, cluster_size, embed_avg
        self.n_q, self.dim, self.size = (int(v) for v in embed.shape)

    @classmethod
    def from_buffers(cls, embeds, cluster_sizes, embed_avgs, device, with_codebook=True):
        """From the reference's per-stage buffers (CPU or device tensors): embed (dim, size), cluster_size (size,) -- None: zeros --,
        embed_avg (dim, size) -- None: a copy of embed --, the defaults VectorQuantize.__init__ registers (vq_module.py:40-43)."""
        emb = [e.detach().float().cpu() for e in embeds]
        cs = [torch.zeros(e.shape[1]) for e in emb] if cluster_sizes is None else [c.detach().float().cpu() for c in cluster_sizes]
        ea = [e.clone() for e in emb] if embed_avgs is None else [a.detach().float().cpu() for a in embed_avgs]
        enorm = torch.stack([e.pow(2).sum(0, keepdim=True)[0] for e in emb])          # as the reference forms it (vq_module.py:96)
        cb = codebook_usage.row_major_codebook(emb, device) if with_codebook else None
        return cls(torch.stack(emb).contiguous().to(device), enorm.contiguous().to(device), cb,
                   torch.stack(cs).contiguous().to(device), torch.stack(ea).contiguous().to(device))


def update(state, z, idx, decay=0.8, eps=1e-5):
    """adk_rvq_ema_update on the current stream of the state's device; does not synchronise.  z (n_rows, dim) float32 and idx
    (n_q, n_rows) int64 (emitted indices, stage offset included), both contiguous on that device.  Overwrites state.embed / enorm /
    codebook (if not None) / cluster_size / embed_avg in place."""
    dev = state.embed.device
    n_q, dim, size = state.n_q, state.dim, state.size
    if z.dim() != 2 or z.shape[1] != dim:
        raise ValueError(f"update: z must be (n_rows, {dim}), got {tuple(z.shape)}")
    n_rows = int(z.shape[0])
    if tuple(idx.shape) != (n_q, n_rows):
        raise ValueError(f"update: idx must be ({n_q}, {n_rows}), got {tuple(idx.shape)}")
    shapes = dict(embed=(n_q, dim, size), enorm=(n_q, size), codebook=(n_q * size, dim), cluster_size=(n_q, size), embed_avg=(n_q, dim, size))
    for name, t, dtype, shape in [("z", z, torch.float32, None), ("idx", idx, torch.int64, None)] + \
            [(k, getattr(state, k), torch.float32, v) for k, v in shapes.items() if getattr(state, k) is not None]:
        # the library takes raw pointers: anything else than this reads garbage or out of bounds
        if t.dtype != dtype or not t.is_contiguous() or t.device != dev or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"update: {name} must be a contiguous {dtype} tensor on {dev}" + (f" of shape {shape}" if shape else "")
                             + f", got {t.dtype} {tuple(t.shape)} on {t.device}, contiguous: {t.is_contiguous()}")
    lib = native.lib()
    ws_bytes = int(lib.adk_rvq_ema_workspace_bytes(n_rows, state.n_q, state.dim, state.size))
    if ws_bytes < 0:
        native.check(ws_bytes, "adk_rvq_ema_workspace_bytes")
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
    native.check(lib.adk_rvq_ema_update(
        _ptr(z), _ptr(idx), n_rows, state.n_q, state.dim, state.size, float(decay), float(eps), _ptr(state.embed), _ptr(state.enorm),
        _ptr(state.codebook), _ptr(state.cluster_size), _ptr(state.embed_avg), _ptr(ws), native.current_stream(dev)), "adk_rvq_ema_update")


def search(state, zt, zq=None):
    """adk_rvq_encode of zt (n_rows, dim) on the state's table: idx (n_q, n_rows) int64, stage offset included; zq (n_rows, dim) is
    written if given."""
    dev = state.embed.device
    idx = torch.empty(state.n_q, zt.shape[0], dtype=torch.int64, device=dev)
    native.check(native.lib().adk_rvq_encode(_ptr(zt), _ptr(state.embed), _ptr(state.enorm), _ptr(idx), _ptr(zq), zt.shape[0],
                                             state.n_q, state.dim, state.size, native.current_stream(dev)), "adk_rvq_encode")
    return idx


def stats(state, zt, idx):
    """(vqloss (n_q,), perplexity (n_q,)) of these rows against the state's CURRENT table (adk_rvq_stats), as device tensors."""
    dev = state.embed.device
    vq = torch.empty(state.n_q, dtype=torch.float32, device=dev)
    ppl = torch.empty(state.n_q, dtype=torch.float32, device=dev)
    acc = codebook_usage.accumulator(state.n_q, state.size, dev)
    codebook_usage.fold(acc, zt, state.codebook, idx, state.n_q, state.dim, state.size, vq, ppl)
    return vq, ppl


class CodebookEMA:
    """EMA re-estimation of an ``AutoEncoderStreamGenerator``'s codebook, on its device.

    Takes ``embed``, ``cluster_size`` and ``embed_avg`` of every stage from the generator's loaded state dict; ``decay`` and ``eps``
    default to ``VectorQuantize``'s (0.8, 1e-5: what ``Quantizer`` constructs).

    ``update(z, idx=None)`` folds the latents ``z`` (B, code_dim, T) -- what ``encode`` returned -- into the statistics and rewrites
    the table, one library call on the current stream, no synchronisation.  Without ``idx`` the search runs here, on the current
    (updated) table; with ``idx`` (n_q, B, T) or (n_q, T) -- what ``quantize`` returned for them -- those codes are used.  Results of
    guarded direct calls are verified first (their call log is settled) and the update itself is never a logged call, so a guard
    repair can never apply an update twice.  Returns ``(vqloss, perplexity)`` of the batch against the OLD table, as the
    reference's training forward returns them (device tensors).

    ``install(generator=None)`` makes a generator (default: the one this object was made from; pass the receiver's too, transmitter
    and receiver each hold their own) use the updated table for ``quantize``, ``quantizer_forward``, ``lookup``, ``lookup_packed``
    and ``forward``.  ``state_dict()`` returns the ``quantizer.codebook.layers.{i}.{embed,cluster_size,embed_avg}`` tensors on the
    CPU: loadable by the reference and by ``load_state_dict`` here.  ``steps()`` counts the updates since the last ``reset()``, which
    reloads the statistics from the generator.

    A ``CodebookUsage`` built before an ``install`` keeps counting against the table it copied: build a new one afterwards."""

    def __init__(self, generator, decay=0.8, eps=1e-5):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"CodebookEMA: decay must be in [0, 1), got {decay}")
        if not float(eps) > 0.0:
            raise ValueError(f"CodebookEMA: eps must be positive, got {eps}")
        self.generator, self.decay, self.eps = generator, float(decay), float(eps)
        self.n_q, self.dim, self.size = generator.n_q, generator.dim, generator.size
        self.device = generator._dev()
        self.reset()

    def reset(self):
        sd = self.generator._sd
        if sd is None:
            raise native.NativeError("CodebookEMA: the generator has no weights (load_state_dict first)")
        self.generator.settle()
        pre = "quantizer.codebook.layers.{}.{}"
        get = lambda name: [sd[pre.format(i, name)] for i in range(self.n_q)] if pre.format(0, name) in sd else None   # noqa: E731
        self.state = State.from_buffers(get("embed"), get("cluster_size"), get("embed_avg"), self.device)
        self._steps = 0
        self._installed = weakref.WeakKeyDictionary({self.generator: 0})      # generator -> steps() when it last got this table
        return self

    def installed_in(self, generator):
        """True if `generator` uses this object's CURRENT table as far as this object knows: it was loaded from it by reset() or
        written into it by install(), and no update has followed.  (A load_state_dict on the generator since then is not seen.)"""
        return self._installed.get(generator) == self._steps

    def steps(self):
        return self._steps

    def _rows(self, z, idx):
        z, idx = lazy_guard.settled(z), lazy_guard.settled(idx)
        if z.dim() != 3 or z.shape[1] != self.dim:
            raise ValueError(f"update: z must be (B, {self.dim}, T), got {tuple(z.shape)}")
        B, D, T = z.shape
        if B * T == 0:
            raise ValueError("update: no rows (the reference's update of an empty batch divides by zero on a fresh codebook)")
        if idx is not None:
            idx = idx.to(device=self.device, dtype=torch.int64)
            if idx.dim() == 2:
                idx = idx.unsqueeze(1)
            if tuple(idx.shape) != (self.n_q, B, T):
                raise ValueError(f"update: idx must be ({self.n_q}, {B}, {T}) for z {tuple(z.shape)}, got {tuple(idx.shape)}")
            idx = idx.reshape(self.n_q, B * T).contiguous()
        zt = z.to(device=self.device, dtype=torch.float32).transpose(2, 1).reshape(B * T, D).contiguous()
        return zt, idx

    def update(self, z, idx=None):
        zt, idx = self._rows(z, idx)
        if idx is None:
            idx = search(self.state, zt)
        vq, ppl = stats(self.state, zt, idx)
        update(self.state, zt, idx, self.decay, self.eps)
        self._steps += 1
        return vq, ppl

    def install(self, generator=None):
        """Device-to-device copy of the table into the generator's search and lookup tensors, after its settle(); the generator's CPU
        state dict is updated as well (this synchronises), so a later configure() / set_*() does not fall back to the old codes."""
        g = generator if generator is not None else self.generator
        if (g.n_q, g.dim, g.size) != (self.n_q, self.dim, self.size):
            raise ValueError(f"install: the generator's quantizer is {g.n_q} x {g.size} x {g.dim}, this table {self.n_q} x {self.size} x {self.dim}")
        if g._sd is None:
            raise native.NativeError("install: the generator has no weights (load_state_dict first)")
        g.settle()
        embed, enorm = g._quantizer()
        if g._codebook is None:
            g.initial()
        embed.copy_(self.state.embed)
        enorm.copy_(self.state.enorm)
        g._codebook.copy_(self.state.codebook)
        g._sd.update(self.state_dict())
        self._installed[g] = self._steps
        return self

    def state_dict(self):
        out = {}
        for name, t in (("embed", self.state.embed), ("cluster_size", self.state.cluster_size), ("embed_avg", self.state.embed_avg)):
            host = t.cpu()
            for i in range(self.n_q):
                out[f"quantizer.codebook.layers.{i}.{name}"] = host[i].clone()
        return out
