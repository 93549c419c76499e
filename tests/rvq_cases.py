"""Operands for which the residual-VQ search (adk_rvq_encode, audiodec_amd/csrc/rvq.hip) has one right answer, at every kind of shape the entry
point accepts -- a plain helper module for tests/test_rvq_shapes.py (CPU: the cases are sharp) and tests/test_gpu_rvq_shapes.py.

Exact cases.  Latents and codes are integers with |v| <= VMAX = 3.  The residual entering stage k is a latent minus k codes, so |r| <= VMAX (k + 1)
per component, and with R = VMAX * n_q the terms of a distance are integers bounded by

    |r|^2 <= dim R^2,    |2 r.E| <= 2 dim R VMAX (every partial sum of the chain too),    |E|^2 <= dim VMAX^2

and every distance by their sum: below 2^24 for dim <= 128 and n_q <= 17 (bound(), asserted), hence exactly representable in f32 whatever the
order of summation.  q' = r + (q - r) = q and r - q' are exact as well.  So the kernel has no rounding to hide behind: its indices must equal the
int64 arg-min with the lowest index among equal distances (np.argmin; `(-dist).max(1)` of the reference, layers/vq_module.py:98), its zq the plain
sum of the chosen codes, bit for bit.  search() is that restatement; with wrong=... it is one of the searches a broken kernel would perform, which
tests/test_rvq_shapes.py requires to be told apart from the right one by these very cases.

Ties.  Low-dimensional cases tie all the time by themselves.  Where the positions exist, stage 0 holds duplicate codes inside one wave of the search
(3, 20), across a wave boundary (63, 64), in the same thread of successive 1024-code slabs (c, c + 1024) and at the last code (p, size - 1; p in
the same, possibly ragged, last wave), and every even row sits exactly on one of them: it ties at distance 0 and leaves the residual 0.  Stages
1.. hold the all-zero code twice, at one of those pairs in turn (the slab pair first): a zero residual ties there, at distance 0 again, and stays
zero -- so a planted row ties at EVERY stage, each time at another kind of position.  Odd rows are random; the codes of stages 1.. are drawn from
{-1, 0, 1}, so that a random row's residual still finds a real code nearer than the planted zero (asserted) and every stage's dot products decide.  Where the last wave holds a single code
(size % 64 == 1) that code stays unique in stage 0 and a row sits on it instead (then the slab pair of size 1025 would be that same code: it is
planted from stage 1 on only).  exact_case() asserts what the tests rely on: the bounds, the share of tied decisions, a tie between c and c + 1024
in every multi-slab case, a winner in the ragged last wave wherever there is one.

Real-valued cases.  Gaussian operands against oracle.rvq_forward_index, under the rules of the existing RVQ tests: indices equal unless the oracle's
own top-2 margin is below MARGIN, zq within ZQ_TOL where the indices agree; real_case() asserts that at most MAX_EXCUSED of the decisions could be
excused at all."""
import numpy as np
import torch

VMAX = 3
SLAB, WAVE = 1024, 64           # codes per pass of the general kernel's 1024 threads; codes per wave of it
RVQ_DIM_MAX = 128

EXACT_SHAPES = [(1, 1, 2), (3, 2, 1), (3, 63, 3), (4, 64, 3), (5, 65, 3), (16, 1000, 3), (17, 1023, 2), (40, 100, 5), (64, 1024, 8),
                (64, 1025, 2), (65, 256, 17), (100, 2049, 2), (128, 1024, 3), (128, 3000, 2)]
ROWS = (1, 3, 4, 5, 9)          # 1, 3, 4, 1, 1 live rows in the last 4-row workgroup
POOL = max(ROWS)
MIN_TIED = 0.05

REAL_SHAPES = [(40, 100, 5), (128, 1500, 3), (65, 256, 16)]
REAL_ROWS = 300
MARGIN, ZQ_TOL, MAX_EXCUSED = 1e-4, 1e-5, 0.005

WRONG = ("highest_index_on_ties", "later_slab_on_ties", "ragged_wave_ignored", "dims_from_64_ignored", "dims_past_16s_ignored",
         "residual_not_updated", "stage0_codebook_everywhere")


def case_id(shape):
    return "x".join(str(v) for v in shape)


def bound(dim, n_q, vmax=VMAX):
    """Upper bound of |distance| and of every intermediate of it, for integer operands with |v| <= vmax (module docstring)."""
    R = vmax * n_q
    return dim * R * R + 2 * dim * R * vmax + dim * vmax * vmax


assert bound(RVQ_DIM_MAX, 17) < 2 ** 24


def search(x, embeds, wrong=None):
    """The residual-VQ search in int64: x (N, dim), embeds [(dim, size)] * n_q, integer-valued -> (indices (n_q, N) within their stage,
    sum of the chosen codes (N, dim), tied (n_q, N, size): the codes at the minimum distance of each decision).  `wrong`: one of WRONG."""
    x = np.asarray(x).astype(np.int64)
    E = [np.asarray(e).astype(np.int64) for e in embeds]
    n, dim = x.shape
    r, zq = x.copy(), np.zeros_like(x)
    idx, tied = [], []
    for st in range(len(E)):
        e = E[0] if wrong == "stage0_codebook_everywhere" else E[st]
        size = e.shape[1]
        dims = {"dims_from_64_ignored": min(dim, 64), "dims_past_16s_ignored": 16 * (dim // 16)}.get(wrong, dim)
        dist = (r * r).sum(1)[:, None] - 2 * (r[:, :dims] @ e[:dims]) + (e * e).sum(0)[None, :]
        codes = np.arange(size)
        if wrong == "ragged_wave_ignored":
            codes = codes[:WAVE * (size // WAVE)]
        if len(codes) == 0:
            best = np.zeros(n, np.int64)
            t = np.zeros((n, size), bool)
        else:
            d = dist[:, codes]
            t = np.zeros((n, size), bool)
            t[:, codes] = d == d.min(1, keepdims=True)
            if wrong == "highest_index_on_ties":
                best = size - 1 - np.argmax(t[:, ::-1], 1)
            elif wrong == "later_slab_on_ties":        # the merge of a thread's successive slabs takes >= instead of >
                last = (size - 1 - np.argmax(t[:, ::-1], 1)) // SLAB
                best = np.argmax(t & (codes[None, :] // SLAB == last[:, None]), 1)
            else:
                best = np.argmax(t, 1)                 # == np.argmin(dist, 1): the lowest index among the minima
                if wrong is None:
                    assert np.array_equal(best, np.argmin(dist, 1))
        q = e[:, best].T
        if wrong != "residual_not_updated":
            r = r - q
        zq = zq + q
        idx.append(best)
        tied.append(t)
    return np.stack(idx), zq, np.stack(tied)


def planted_pairs(size):
    """{kind: (lower, higher)}: the duplicate positions that exist at this codebook size."""
    p = {}
    if size > 20:
        p["wave"] = (3, 20)
    if size > WAVE:
        p["boundary"] = (WAVE - 1, WAVE)
    if size > SLAB:
        c = min(5, size - SLAB - 1)
        p["slab"] = (c, c + SLAB)
    if size >= 63:
        last0 = WAVE * ((size - 1) // WAVE)            # first code of the last wave (that wave holds size - 1 alone: a code of the wave before)
        p["last"] = (last0 if last0 < size - 1 else size - 41, size - 1)
    return p


class ExactCase:
    """x (rows, dim) and embeds [(dim, size)] * n_q as float32 tensors; idx (n_q, rows) int64 within the stage, zq (rows, dim) float32 and
    tied (n_q, rows, size) bool: the exact answer.  Rows are independent: the answer for x[:n] is idx[:, :n], zq[:n]."""

    def __init__(self, shape, rows, x, embeds):
        self.shape, self.rows = shape, rows
        self.dim, self.size, self.n_q = shape
        self.x, self.embeds = x, embeds
        idx, zq, self.tied = search(x.numpy(), [e.numpy() for e in embeds])
        self.idx = torch.from_numpy(idx)
        self.zq = torch.from_numpy(zq).float()
        self.offsets = (torch.arange(self.n_q) * self.size).view(-1, 1)

    def decisions(self):
        return self.n_q * self.rows

    def tied_share(self):
        return float((self.tied.sum(2) >= 2).mean())


_SEEDS = {(3, 2, 1): 18}        # two codes in three dimensions: a draw in which two of the nine rows are equidistant and both codes win


def exact_case(shape, rows=POOL):
    dim, size, n_q = shape
    g = torch.Generator().manual_seed(_SEEDS.get(tuple(shape), 0) + 1000003 * dim + 1009 * size + n_q)

    def draw(vmax, *s):
        return torch.randint(-vmax, vmax + 1, s, generator=g).float()

    embeds = [draw(VMAX if st == 0 else 1, dim, size) for st in range(n_q)]
    x = draw(VMAX, rows, dim)
    pairs = planted_pairs(size)
    single_last = size > 1 and size % WAVE == 1         # the last wave holds one code: it stays unique in stage 0
    stage0 = {k: v for k, v in pairs.items() if not (single_last and (k == "last" or v[1] == size - 1))}
    for lo, hi in stage0.values():
        embeds[0][:, hi] = embeds[0][:, lo]
    later = [pairs[k] for k in ("slab", "last", "boundary", "wave") if k in pairs]
    for st in range(1, n_q):
        if later:
            lo, hi = later[(st - 1) % len(later)]
            embeds[st][:, lo] = 0.0
            embeds[st][:, hi] = 0.0
    sit_on = [hi for _, hi in stage0.values()] + ([size - 1] if single_last else [])
    for i in range(0, rows, 2):
        if sit_on:
            x[i] = embeds[0][:, sit_on[(i // 2) % len(sit_on)]]
    case = ExactCase(tuple(shape), rows, x, embeds)
    check_exact_case(case, stage0, later, sit_on)
    return case


def check_exact_case(case, stage0, later, sit_on):
    """What the tests rely on (module docstring), asserted from the operands and the exact answer."""
    dim, size, n_q = case.shape
    what = case_id(case.shape)
    ops = [case.x] + case.embeds
    assert all(torch.equal(o, o.round()) and float(o.abs().max()) <= VMAX for o in ops), what
    assert n_q <= 17 and dim <= RVQ_DIM_MAX and bound(dim, n_q) < 2 ** 24, what
    # ... and the bound is one: the residuals and distances that actually occur stay under it
    r = case.x.numpy().astype(np.int64)
    for st, e in enumerate(case.embeds):
        e = e.numpy().astype(np.int64)
        assert np.abs(r).max() <= VMAX * (st + 1), what
        assert (r * r).sum(1).max() + 2 * (np.abs(r) @ np.abs(e)).max() + (e * e).sum(0).max() < 2 ** 24, what
        r = r - e[:, case.idx[st].numpy()].T
    n_tied = case.tied.sum(2)
    if size > 1:                                                    # (one code cannot tie with another)
        assert case.tied_share() >= MIN_TIED, (what, case.tied_share())
    win = case.idx.numpy()
    if size > SLAB:                                                 # the same thread's candidates of two successive slabs tie, the earlier wins
        assert (case.tied[np.arange(n_q)[:, None], np.arange(case.rows)[None, :], np.minimum(win + SLAB, size - 1)]
                & (win + SLAB < size)).any(), what
    if size % WAVE:
        assert (win >= WAVE * (size // WAVE)).any(), what
    if dim >= 16 and n_q > 1 and case.rows > 1:
        # the random rows keep deciding between real codes after stage 0: the later stages' codes are drawn from {-1, 0, 1}, small enough against
        # the residual that the planted all-zero code does not swallow them (2 max r.E > |E|^2)
        live = [bool(case.embeds[st][:, win[st, i]].any()) for st in range(1, n_q) for i in range(1, case.rows, 2)]
        assert np.mean(live) >= 0.75, (what, np.mean(live))
    if dim >= 64:                                                   # every planted pair ties where a row sits on it, the lower index wins
        for i in range(0, case.rows, 2):
            if not sit_on:
                break
            hi = sit_on[(i // 2) % len(sit_on)]
            lo = [l for l, h in stage0.values() if h == hi]
            assert case.tied[0, i, hi] and int(win[0, i]) == (lo[0] if lo else hi), (what, i)
            assert not lo or case.tied[0, i, lo[0]], (what, i)
            for st in range(1, n_q):
                l, h = later[(st - 1) % len(later)]
                assert int(win[st, i]) == l and case.tied[st, i, h] and n_tied[st, i] == 2, (what, i, st)
            assert not case.zq[i].ne(case.x[i]).any(), (what, i)     # the residual stayed zero: zq is the row


class RealCase:
    """x (1, rows, dim), embeds, and the oracle's zq (1, rows, dim), idx (n_q, rows) within the stage, margin (n_q, rows)."""

    def __init__(self, shape, x, embeds):
        from oracle import audiodec_oracle as O
        self.shape = shape
        self.dim, self.size, self.n_q = shape
        self.x, self.embeds = x, embeds
        self.zq, self.idx, self.margin = O.rvq_forward_index(x, embeds, flatten_idx=False, return_margin=True)
        self.offsets = (torch.arange(self.n_q) * self.size).view(-1, 1)
        self.excusable = self.margin < MARGIN
        self.excusable_share = float(self.excusable.float().mean())


def real_case(shape, rows=REAL_ROWS, seed=20240):
    dim, size, n_q = shape
    g = torch.Generator().manual_seed(seed + 1000003 * dim + 1009 * size + n_q)
    embeds = [torch.randn(dim, size, generator=g) * (0.8 ** i) for i in range(n_q)]
    x = torch.randn(1, rows, dim, generator=g)
    case = RealCase(tuple(shape), x, embeds)
    assert all(bool(torch.isfinite(t).all()) for t in (case.zq, case.margin)), case_id(shape)
    assert case.excusable_share <= MAX_EXCUSED, (case_id(shape), case.excusable_share)
    return case


def check_real(case, zq, idx, what):
    """The existing RVQ rules (module docstring) for a kernel's zq (1, rows, dim) and in-stage idx (n_q, rows); returns the excused share."""
    differ = idx != case.idx
    assert not bool((differ & ~case.excusable).any()), (what, np.argwhere((differ & ~case.excusable).numpy())[:5])
    same = ~differ.any(0)
    err = float((zq[0, same] - case.zq[0, same]).abs().max())
    assert err <= ZQ_TOL, (what, err)
    return float(differ.float().mean())
