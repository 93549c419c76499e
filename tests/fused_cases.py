"""The two fused vocoder-tail launches as mini-programs, an exact model of each pair, and an f32 emulation that can be made wrong on purpose.

Plain helper for tests/test_fused_cases.py (CPU) and tests/test_gpu_fused_exact.py (GPU); importing it needs no GPU.

THE PROGRAMS.  program.Builder with a synthetic state dict and hand-made arch.ConvSpecs:
    ring write from ext[0] -> op A (1x1 conv, fuse_next) -> op B -> copy to an external ring (b.mean([x], out))
  pair `ou` (csrc/conv_ou16.hip):  A = 192 -> 64, no activation;  B = convT 64 -> cout_real, stride `up`, input activation `act`;
  pair `oc` (csrc/conv_oc16.hip):  A = 96 -> 32;  B = conv 32 -> 1, K 7, input activation `act`, act_out tanh or none (IMPL_AUTO: one output
  channel has no matrix-core form, as op_pair_kind requires).
The fused twin leaves fuse_next = 1 on A, the two-launch twin clears it; same weights, same arena.  Every ring is history + one full step
(max frames x rate), the output ring of B is internal (its cursor wraps; out_hist > 0 makes its row count no multiple of `up`, so the phases
of one step straddle the wrap).  T = rate x frames of the call.

THE EXACT MODEL.  The argument of tests/split16_model.py and tests/chain_cases.py carried through two convs.
  node c = W1 x + b1 minus the dropped lo*lo term (split16_model.evaluate): x on a grid of unit ux, W1 of unit uw1 (1: integers, 2^-14:
  two-level n + m 2^-14), so c is a multiple of q1 = ux uw1, and S1 = sum |x| |w1| + |b1| < 2^23 q1 makes every partial sum exact.
  ou:  the kernel splits act(c) AGAIN into f16 hi / lo: act(c) must equal its own split (asserted), which caps |c| near 2^8 where it carries
       2^-14 fractions.  qa = q1 (no activation, ELU or LeakyReLU on non-negative data) or q1 * slope; W2 of unit uw2; q2 = qa uw2;
       S2 = sum |act(c)| |w2| + |b2| < 2^23 q2.  bias 2 repeats per phase, the transposed conv crops as split16_model._convtr_map does.
  oc:  the second conv is plain f32 fmaf on act(c) and the UNSPLIT weights (integers or signed powers of two: unit 1): every fma is exact
       while sum |w| |act(c)| + |b| < 2^24 qa.
  Budget: a two-level operand costs 14 bits from its conv on, a LeakyReLU on signed data log2(1 / slope) bits.  Kinds:
    `w1two`  two-level W1 (non-negative), small integer x, sparse integer W2;
    `xtwo`   two-level x, integer W1 / W2;
    `w2two`  (ou) two-level W2 on small integer c;
    `signed` integers of both signs, |x| <= 3000, 12 weights +-1 per row of W1: c passes 2^11, so the lo half of x is live in GEMM 1 and
             that of act(c) in GEMM 2; slope 0.5 or 0.25.
run_model ASSERTS before any kernel runs: operands equal to their split, every S under its cap (the largest share is reported), every node
on its grid and representable, >= 90 % of every call's outputs and of the stored history rows non-zero, the lo halves a kind is about live.

THE CALL PROTOCOL.  chain_cases.protocol: >= 6 calls of mixed frame counts, the last stream's rings zeroed half-way
(restore_stream_state(B - 1, None)), one whole-program reset; streams carry classes (chain_cases.stream_classes).  After every call: the
output, the live history rows of c (RAW, not activated: one for ou, six for oc) and the program's flag word."""
import functools

import torch
import torch.nn.functional as F

import chain_cases as CC
import split16_model as M

PAIRS = {"ou": dict(cin=192, cm=64, hist=1), "oc": dict(cin=96, cm=32, hist=6)}
OU_TMAX, OC_SLMAX = 128, 122
# every (up, cout_real) conv_up16_supported admits: up > 1, cout_real % 4 == 0, up * cout_real in {32, 64, 96}
ADMITTED = [(up, g // up) for g in (32, 64, 96) for up in range(2, g + 1) if g % up == 0 and (g // up) % 4 == 0]
OU_LADDER = [128, 1, 100, 2, 15, 127, 16, 17, 128]              # a short call's history row feeds a long call
OC_LADDER_A = [366, 5, 1, 2, 300, 6, 245, 1, 244, 7, 27]        # 5 + 1 + 2: the six-step history of the T = 300 call comes from three calls
OC_LADDER_B = [123, 26, 1, 122, 2, 1, 1, 121, 27, 5, 123]
SHORT = [33, 17, 33, 1, 16, 33, 2]


def case(pair, name, B, frames, rate=1, up=3, cout=32, act="LeakyReLU", kind="signed", slope=0.5, b1=True, b2=True, act_out=None, out_hist=0,
         seed=0):
    """One case.  b2: bias of op B; act: None | 'LeakyReLU' | 'ELU' (input activation of B); act_out (oc): None | 'tanh'."""
    assert pair in PAIRS and kind in ("signed", "w1two", "xtwo", "w2two") and (kind != "w2two" or pair == "ou")
    assert act != "ELU" or kind != "signed", "ELU stays exact only on non-negative data"
    if pair == "oc":
        up, cout = 1, 1
    return dict(pair=pair, name=name, B=B, frames=list(frames), rate=rate, F=max(frames), up=up, cout=cout, act=act, kind=kind,
                slope=slope if act == "LeakyReLU" else 0.0, b1=b1, b2=b2, act_out=act_out, out_hist=out_hist, seed=seed)


def _key(c):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in c.items()))


def slices(T):
    """(number of slices, steps per slice) of launch_conv_oc16."""
    n = -(-T // OC_SLMAX)
    sl = -(-T // n)
    return -(-T // sl), sl


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def _sparse(g, rows, cols, fan, values):
    idx = torch.rand(rows, cols, generator=g).argsort(1)[:, :fan]
    w = torch.zeros(rows, cols, dtype=torch.float64)
    w.scatter_(1, idx, values(idx.shape))
    return w


@functools.lru_cache(maxsize=None)
def _operands_cached(key):
    c = dict(key)
    g = torch.Generator().manual_seed(2000 + c["seed"])
    P, kind, ou = PAIRS[c["pair"]], c["kind"], c["pair"] == "ou"
    signed = kind == "signed"
    sign = lambda s: (torch.randint(0, 2, s, generator=g) * 2 - 1).double()
    ones = lambda s: torch.ones(s, dtype=torch.float64)
    two = lambda s: torch.randint(1, 3, s, generator=g).double() + torch.randint(1, 4, s, generator=g).double() * sign(s) * M.UNIT
    ints = lambda s: torch.randint(1, 3, s, generator=g).double()
    fan1 = 12 if signed else ({"w1two": 16, "xtwo": 12, "w2two": 3}[kind] if ou else {"w1two": 4, "xtwo": 6}[kind])
    w1 = _sparse(g, P["cm"], P["cin"], fan1, sign if signed else (two if kind == "w1two" else ones)).view(P["cm"], P["cin"], 1).float()

    def bias(n):
        b = torch.randint(1, 5, (n,), generator=g).double()
        return (b * sign((n,)) if signed else b).float()

    b1 = bias(P["cm"]) if c["b1"] else None
    if ou:
        up, co = c["up"], c["cout"]
        fan2 = 3 if signed else (4 if kind == "w2two" else 2)
        wt = _sparse(g, co * 2 * up, 64, fan2, sign if signed else (two if kind == "w2two" else ints))       # row (co, kk) over ci
        w2 = wt.view(co, 2 * up, 64).permute(2, 0, 1).contiguous().float()                                    # ConvTranspose1d: (ci, co, kk)
        b2 = bias(co) if c["b2"] else None
    else:
        if signed:
            wt = (2.0 ** torch.randint(0, 3, (7, 32), generator=g).double()) * sign((7, 32))                 # dense, +-{1, 2, 4}
        else:
            wt = _sparse(g, 7, 32, 2, ints)                                                                   # two weights per tap
        w2 = wt.t().contiguous().view(1, 32, 7).float()
        b2 = bias(1) if c["b2"] else None
    _, ncls = CC.stream_classes(c["B"])
    xs = []
    for f, _, _ in CC.protocol(c):
        shape = (ncls, P["cin"], f * c["rate"])
        if signed:
            x = (torch.randint(1, 3001, shape, generator=g).double() * sign(shape)).float()
        elif kind == "xtwo":
            x = M.grid(g, shape, 3, signed=False)
        else:
            x = torch.randint(1, 4, shape, generator=g).float()
        xs.append(x)
    return (w1, b1, w2, b2), xs


def operands(c):
    """((W1 (cm, cin, 1), b1, W2, b2), per-call inputs [(classes, cin, T)]); W2: ou (64, cout_real, 2 up) as ConvTranspose1d holds it, oc (1, 32, 7)."""
    return _operands_cached(_key(c))


def real_operands(c):
    """Gaussian weights, biases and inputs of both signs for the case's shapes: no model; ELU's negative side and slope 0.01 live."""
    g = torch.Generator().manual_seed(7000 + c["seed"])
    P = PAIRS[c["pair"]]
    w1 = torch.randn(P["cm"], P["cin"], 1, generator=g) * (1.0 / P["cin"] ** 0.5)
    b1 = torch.randn(P["cm"], generator=g) * 0.1 if c["b1"] else None
    if c["pair"] == "ou":
        w2 = torch.randn(64, c["cout"], 2 * c["up"], generator=g) * (0.7 / 128 ** 0.5)
        b2 = torch.randn(c["cout"], generator=g) * 0.1 if c["b2"] else None
    else:
        w2 = torch.randn(1, 32, 7, generator=g) * (0.7 / 224 ** 0.5)
        b2 = torch.randn(1, generator=g) * 0.1 if c["b2"] else None
    _, ncls = CC.stream_classes(c["B"])
    xs = [torch.randn(ncls, P["cin"], f * c["rate"], generator=g) for f, _, _ in CC.protocol(c)]
    return (w1, b1, w2, b2), xs


# ------------------------------------------------------------------------------------------------
# the exact model
# ------------------------------------------------------------------------------------------------
def _conv1(a, w):
    return F.conv1d(a, w)


def second_conv(c, win, w2, b2, qa):
    """Op B on the raw window (history in front) in f64: (pre-activation output, S2 as a share of its cap, share of act(c) with a live lo half)."""
    if c["pair"] == "ou":
        q2 = qa * (M.UNIT if c["kind"] == "w2two" else 1.0)
        p = M.parts(win, w2, c["act"], c["slope"])                                     # (combine asserts act(c) == its own split)
        y, _, s2 = M.combine(M._convtr_map(c["up"]), *p, b2, None, q2)
        return y, s2 / (2.0 ** 23 * q2), float((p[2] != 0).double().mean())
    a = M.act64(win, c["act"], c["slope"])
    assert bool((a.float().double() == a).all())
    w = w2.double()
    assert bool((w == w.round()).all()), "the output conv's weights are integers (unit 1)"
    y = F.conv1d(a, w) + (0.0 if b2 is None else b2.double().view(1, 1, 1))
    S = F.conv1d(a.abs(), w.abs()) + (0.0 if b2 is None else b2.double().abs().view(1, 1, 1))
    assert float(S.max()) < 2.0 ** 24 * qa, f"S2 = {float(S.max())} is not below the cap {2.0 ** 24 * qa}"
    assert bool((y.float().double() == y).all()) and bool(((y / qa).round() * qa == y).all()), "the output is off its grid"
    return y.float(), float(S.max()) / (2.0 ** 24 * qa), 0.0


@functools.lru_cache(maxsize=None)
def _model_cached(key):
    c = dict(key)
    (w1, b1, w2, b2), xs = _operands_cached(key)
    P, kind = PAIRS[c["pair"]], c["kind"]
    _, ncls = CC.stream_classes(c["B"])
    hk = P["hist"]
    hist = torch.zeros(ncls, P["cm"], hk, dtype=torch.float64)
    q1 = M.UNIT if kind in ("w1two", "xtwo") else 1.0
    calls, share, lo_x, lo_a = [], 0.0, [], []
    filled, stored, stored_nz = [0] * ncls, 0, 0
    for (f, zero_last, reset), x in zip(CC.protocol(c), xs):
        if reset:
            hist.zero_()
            filled = [0] * ncls
        if zero_last:
            hist[ncls - 1] = 0
            filled[ncls - 1] = 0
        T = f * c["rate"]
        filled = [v + T for v in filled]
        p = M.parts(x, w1, None, 0.0)
        node, _, s1 = M.combine(_conv1, *p, b1, None, q1)
        share = max(share, s1 / (2.0 ** 23 * q1))
        lo_x.append(float((p[2] != 0).double().mean()))
        win = torch.cat([hist, node.double()], 2)
        nonneg = bool((win >= 0).all())
        assert c["act"] != "ELU" or nonneg, f"{c['name']}: a negative ELU input"
        qa = q1 * c["slope"] if (c["act"] == "LeakyReLU" and not nonneg) else q1
        pre, sh2, la = second_conv(c, win, w2, b2, qa)
        share = max(share, sh2)
        lo_a.append(la)
        assert float((pre != 0).float().mean()) >= 0.9, f"{c['name']}: a call's outputs are mostly zero"
        out = torch.tanh(pre) if c["act_out"] == "tanh" else pre
        hist = win[:, :, win.shape[2] - hk:].clone()
        for cl in range(ncls):
            part = hist[cl, :, hk - min(hk, filled[cl]):]
            stored += part.numel()
            stored_nz += int((part != 0).sum())
        calls.append(dict(frames=f, T=T, zero_last=zero_last, reset=reset, x=x, out=out, pre=pre, hist=hist.float()))
    assert stored_nz >= 0.9 * stored, f"{c['name']}: the stored history of c is mostly zero"
    lo_w1, lo_w2 = float((M.split(w1)[1] != 0).float().mean()), float((M.split(w2)[1] != 0).float().mean())
    lo_x, lo_a = sum(lo_x) / len(lo_x), sum(lo_a) / len(lo_a)
    if kind == "signed":
        assert lo_x >= 0.05 and (c["pair"] == "oc" or lo_a >= 0.05), (c["name"], lo_x, lo_a)
    if kind == "w1two":
        assert lo_w1 > 0 and lo_w2 == 0 and (c["pair"] == "oc" or lo_a >= 0.25), (c["name"], lo_w1, lo_a)
    if kind == "xtwo":
        assert lo_x >= 0.25 and lo_w1 == 0 and (c["pair"] == "oc" or lo_a >= 0.25), (c["name"], lo_x, lo_a)
    if kind == "w2two":
        assert lo_w2 > 0 and lo_w1 == 0, (c["name"], lo_w2)
    return calls, dict(share=share, lo_x=lo_x, lo_a=lo_a, lo_w1=lo_w1, lo_w2=lo_w2)


def run_model(c):
    """(calls, stats): per call the input, the model's output (classes, ch, T up) -- for act_out tanh the CPU's tanh of the exact
    pre-activation `pre`, which a GPU test does NOT compare bit for bit --, the live history rows of c after it; stats: the largest S as a
    share of its cap and the shares of operands with a live lo half."""
    return _model_cached(_key(c))


def one_hot_w1(c, seed, scale=1.0):
    """(W1, column of every row, sign of every row): one weight +-scale per row, every row another input channel -- c = +-scale * joined(x)."""
    g = torch.Generator().manual_seed(9000 + seed)
    P = PAIRS[c["pair"]]
    perm = torch.randperm(P["cin"], generator=g)[:P["cm"]]
    sgn = (torch.randint(0, 2, (P["cm"],), generator=g) * 2 - 1).float()
    w1 = torch.zeros(P["cm"], P["cin"])
    w1[torch.arange(P["cm"]), perm] = sgn * scale
    return w1.view(P["cm"], P["cin"], 1), perm, sgn


def unchecked_model(c, ops, xs):
    """The model for operands off the grid (the format's edges), nothing asserted: per call (pre-activation output, history rows of c, S of
    the second conv per output), in f64.  No zeroed stream, no reset: the caller's protocol has none."""
    w1, b1, w2, b2 = ops
    hk = PAIRS[c["pair"]]["hist"]
    hist, res = None, []
    for x in xs:
        node = M.evaluate(_conv1, *M.parts(x, w1, None, 0.0), b1, None)[0].float().double()
        hist = torch.zeros(x.shape[0], node.shape[1], hk, dtype=torch.float64) if hist is None else hist
        win = torch.cat([hist, node], 2)
        if c["pair"] == "ou":
            y, _, S = M.evaluate(M._convtr_map(c["up"]), *M.parts(win, w2, c["act"], c["slope"]), b2, None)
        else:
            a = M.act64(win, c["act"], c["slope"])
            bb = 0.0 if b2 is None else b2.double().view(1, 1, 1)
            y, S = F.conv1d(a, w2.double()) + bb, F.conv1d(a.abs(), w2.double().abs()) + abs(bb)
        hist = win[:, :, win.shape[2] - hk:].clone()
        res.append((y, hist, S))
    return res


# ------------------------------------------------------------------------------------------------
# f32 emulation of each launch over explicit rings, right or wrong
# ------------------------------------------------------------------------------------------------
OU_FAULTS = ["halo_late", "halo_skip", "hist_raw", "hist_early", "clast15", "bias2_tile", "phase_cout_g", "swizzle", "drop_alo_whi2",
             "act_lo_dropped", "store_past_T"]
OC_FAULTS = ["lead_from_ring", "slice0_recomputed", "to_ring_short", "hist_activated", "taps_reversed", "last_slice_len", "bias1_on_hist",
             "drop_xlo_whi", "drop_xhi_wlo"]


def pack_convtr(w, up):
    """ConvTranspose1d weight (ci, co, 2 up) -> polyphase GEMM rows [(phase, co)][(tap, ci)], tap 0 = the older row."""
    old, new = w[:, :, up:].permute(2, 1, 0), w[:, :, :up].permute(2, 1, 0)
    return torch.cat([old, new], 2).reshape(up * w.shape[1], 2 * w.shape[0]).contiguous()


def _act32(v, act, slope):
    if act == "ELU":
        return F.elu(v)
    if act == "LeakyReLU":
        return torch.where(v > 0, v, v * slope)
    return v


def _gemm3(a, w, g, shuffle, drop=None, no_alo=False):
    """a (n, R, K), w (M, K) -> (n, R, M): hi*hi, and hi*lo + lo*hi joined as m + c / 2048, the k order shuffled in chunks of 16."""
    ah, al = (t.float() for t in M.split(a))
    wh, wl = (t.float() for t in M.split(w))
    if no_alo:
        al = torch.zeros_like(al)
    K = a.shape[-1]
    order = torch.randperm(K, generator=g) if shuffle else torch.arange(K)
    m = torch.zeros(a.shape[0], a.shape[1], w.shape[0])
    cc = torch.zeros_like(m)
    for i in range(0, K, 16):
        j = order[i:i + 16]
        m = m + ah[..., j] @ wh[:, j].t()
        if drop != "alo_whi":
            cc = cc + al[..., j] @ wh[:, j].t()
        if drop != "ahi_wlo":
            cc = cc + ah[..., j] @ wl[:, j].t()
    return m + cc * (1.0 / 2048.0)


def emulate(c, ops, xs, fault=None, shuffle=True):
    """The case's launch in f32 over explicit rings with cursors, as the kernel of its pair runs it.  fault: one of OU_FAULTS / OC_FAULTS.
    Returns per call (output (classes, ch, T up), live history rows of c (classes, cm, hist))."""
    return (_emulate_ou if c["pair"] == "ou" else _emulate_oc)(c, ops, xs, fault, shuffle)


def _emulate_ou(c, ops, xs, fault, shuffle):
    """conv_ou16: wave w = steps 16 w .. 16 w + 15; rows past T are copies of row T - 1 (the DMA's source is clamped); the older tap of a
    wave's first step is the halo row the wave in front wrote (wave 0: the activated history row); of c only row T - 1 is stored; the
    outputs go to (cursor + t up) % rows + phase, wrapped once, as flat addresses into the output ring (out of the buffer: dropped).
    Faults: halo_late (halo of wave w + 1 from step 16 w + 14), halo_skip (halo written only where the next wave is full), hist_raw, hist_early
    (one ring row early), clast15 (c of step 15 of the last live wave, read past T in the input ring), bias2_tile (bias 2 indexed inside the
    16-row m-tile), phase_cout_g (phase = ml // cout_g), swizzle (two 16-byte pieces of column block 2 swapped), drop_alo_whi2,
    act_lo_dropped, store_past_T (rows past T stored, after the valid ones)."""
    w1, b1, w2, b2 = ops
    g = torch.Generator().manual_seed(78)
    _, ncls = CC.stream_classes(c["B"])
    up, co = c["up"], c["cout"]
    cg = up * co
    step = c["rate"] * c["F"]
    rows_x, rows_c, rows_o = step, 1 + step, c["out_hist"] + step * up
    xr, cr = torch.zeros(ncls, rows_x, 192), torch.zeros(ncls, rows_c, 64)
    orr = torch.zeros(ncls * rows_o * co)
    cur_x = cur_c = cur_o = 0
    wp = pack_convtr(w2, up)
    b2rep = b2.repeat(up) if b2 is not None else torch.zeros(cg)
    ml = torch.arange(cg)
    res = []
    for (f, zero_last, reset), x in zip(CC.protocol(c), xs):
        T = f * c["rate"]
        if reset:
            xr.zero_(); cr.zero_(); orr.zero_()
            cur_x = cur_c = cur_o = 0
        if zero_last:
            cr[ncls - 1, (cur_c - 1) % rows_c] = 0
        xr[:, (cur_x + torch.arange(T)) % rows_x] = x.float().transpose(1, 2)
        nw = -(-T // 16)
        t = torch.arange(16 * nw)
        X = xr[:, (cur_x + t.clamp(max=T - 1)) % rows_x]
        if fault == "swizzle":
            X = X.clone()
            X[:, :, 64:68], X[:, :, 68:72] = X[:, :, 68:72].clone(), X[:, :, 64:68].clone()
        w1m = w1.view(64, 192)
        cc_ = _gemm3(X, w1m, g, shuffle)
        if b1 is not None:
            cc_ = cc_ + b1
        a = _act32(cc_, c["act"], c["slope"])
        hraw = cr[:, (cur_c - (2 if fault == "hist_early" else 1)) % rows_c]
        hact = hraw if fault == "hist_raw" else _act32(hraw, c["act"], c["slope"])
        prev = torch.cat([hact[:, None], a[:, :-1]], 1).clone()
        for w in range(1, nw):
            if fault == "halo_late":
                prev[:, 16 * w] = a[:, 16 * w - 2]
            if fault == "halo_skip" and 16 * (w + 1) > T:
                prev[:, 16 * w] = 0
        y = _gemm3(torch.cat([prev, a], 2), wp, g, shuffle, "alo_whi" if fault == "drop_alo_whi2" else None, fault == "act_lo_dropped")
        y = y + b2rep[(ml % 16) if fault == "bias2_tile" else ml]
        ph = torch.zeros_like(ml) if fault == "phase_cout_g" else ml // co
        r2 = ((cur_o + t * up) % rows_o)[:, None] + ph[None, :]
        r2 = torch.where(r2 >= rows_o, r2 - rows_o, r2)
        flat = (torch.arange(ncls)[:, None, None] * rows_o + r2[None]) * co + (ml - ph * co)[None, None, :]
        ov = orr
        for sel in ([t < T, t >= T] if fault == "store_past_T" else [t < T]):
            fl, yy = flat[:, sel].reshape(-1), y[:, sel].reshape(-1)
            ok = fl < ov.numel()
            ov[fl[ok]] = yy[ok]
        clast = cc_[:, T - 1]
        if fault == "clast15":
            xl = xr[:, (cur_x + 16 * nw - 1) % rows_x][:, None]
            clast = _gemm3(xl, w1m, g, shuffle)[:, 0] + (b1 if b1 is not None else 0.0)
        cr[:, (cur_c + T - 1) % rows_c] = clast
        out = orr.view(ncls, rows_o, co)[:, (cur_o + torch.arange(T * up)) % rows_o]
        cur_x, cur_c, cur_o = (cur_x + T) % rows_x, (cur_c + T) % rows_c, (cur_o + T * up) % rows_o
        res.append((out.transpose(1, 2).contiguous(), cr[:, [(cur_c - 1) % rows_c]].transpose(1, 2).contiguous()))
    return res


def _emulate_oc(c, ops, xs, fault, shuffle):
    """conv_oc16: slice i = steps i sl .. ; its GEMM columns start six steps early; those of slice 0 are the ring's history (raw c of earlier
    calls), those of later slices recomputed from the input rows; raw c of the call's last six steps goes to the ring; the output conv in
    f32, + bias, act_out.  Faults: lead_from_ring, slice0_recomputed (from the clamped input row 0), to_ring_short (t >= T - 5),
    hist_activated, taps_reversed, last_slice_len (the last slice's length as every slice's), bias1_on_hist, drop_xlo_whi / drop_xhi_wlo
    (a cross term of GEMM 1)."""
    w1, b1, w2, b2 = ops
    g = torch.Generator().manual_seed(79)
    _, ncls = CC.stream_classes(c["B"])
    step = c["rate"] * c["F"]
    rows_x, rows_c = step, 6 + step
    xr, cr = torch.zeros(ncls, rows_x, 96), torch.zeros(ncls, rows_c, 32)
    cur_x = cur_c = 0
    wt = w2.view(32, 7).t().contiguous()                                # [tap][channel]
    if fault == "taps_reversed":
        wt = wt.flip(0)
    wflat = wt.reshape(-1)
    drop = {"drop_xlo_whi": "alo_whi", "drop_xhi_wlo": "ahi_wlo"}.get(fault)
    res = []
    for (f, zero_last, reset), x in zip(CC.protocol(c), xs):
        T = f * c["rate"]
        if reset:
            xr.zero_(); cr.zero_()
            cur_x = cur_c = 0
        if zero_last:
            cr[ncls - 1, (cur_c - 6 + torch.arange(6)) % rows_c] = 0
        xr[:, (cur_x + torch.arange(T)) % rows_x] = x.float().transpose(1, 2)
        n, sl = slices(T)
        if fault == "last_slice_len":
            sl = T - (n - 1) * sl
        out = torch.zeros(ncls, T)
        hrows = cr[:, (cur_c - 6 + torch.arange(6)) % rows_c].clone()
        for i in range(n):
            t0 = i * sl
            nt = min(sl, T - t0)
            if nt <= 0:
                continue
            t = t0 - 6 + torch.arange(nt + 6)
            cc_ = _gemm3(xr[:, (cur_x + t.clamp(0, T - 1)) % rows_x], w1.view(32, 96), g, shuffle, drop)
            if b1 is not None:
                cc_ = cc_ + b1
            if i == 0 and fault != "slice0_recomputed":
                cc_[:, :6] = hrows + (b1 if (fault == "bias1_on_hist" and b1 is not None) else 0.0)
            if i > 0 and fault == "lead_from_ring":
                cc_[:, :6] = hrows
            keep = (t >= t0) & (t >= T - (5 if fault == "to_ring_short" else 6))
            cr[:, (cur_c + t[keep]) % rows_c] = _act32(cc_[:, keep], c["act"], c["slope"]) if fault == "hist_activated" else cc_[:, keep]
            a = _act32(cc_, c["act"], c["slope"])
            U = a.unfold(1, 7, 1).permute(0, 1, 3, 2).reshape(ncls, nt, 224)          # [step][tap][channel]
            order = torch.randperm(224, generator=g) if shuffle else torch.arange(224)
            acc = torch.zeros(ncls, nt)
            for k in range(0, 224, 16):
                j = order[k:k + 16]
                acc = acc + (U[..., j] * wflat[j]).sum(-1)
            if b2 is not None:
                acc = acc + b2
            out[:, t0:t0 + nt] = torch.tanh(acc) if c["act_out"] == "tanh" else acc
        cur_x, cur_c = (cur_x + T) % rows_x, (cur_c + T) % rows_c
        res.append((out[:, None].contiguous(), cr[:, (cur_c - 6 + torch.arange(6)) % rows_c].transpose(1, 2).contiguous()))
    return res


# ------------------------------------------------------------------------------------------------
# the programs (GPU)
# ------------------------------------------------------------------------------------------------
def build_program(c, ops, fused, device="cuda:0", act2=None):
    """(HipProgram, ring of c): the fused program (fuse_next = 1 on op A) or its two-launch twin.  act2: op B's input activation code,
    where it is not the case's (the tanh the launch must decline)."""
    from audiodec_amd import arch, native, program
    w1, b1, w2, b2 = ops
    P, ou = PAIRS[c["pair"]], c["pair"] == "ou"
    sa = arch.ConvSpec("a", "conv", P["cin"], P["cm"], 1, 1, 1, 1, b1 is not None)
    sb = (arch.ConvSpec("b", "convT", 64, c["cout"], 2 * c["up"], c["up"], 1, 1, b2 is not None) if ou
          else arch.ConvSpec("b", "conv", 32, 1, 7, 1, 1, 1, b2 is not None))
    sd = {sa.wkey("weight"): w1, sb.wkey("weight"): w2}
    if b1 is not None:
        sd[sa.wkey("bias")] = b1
    if b2 is not None:
        sd[sb.wkey("bias")] = b2
    b = program.Builder(sd, [sa, sb], split16=True)
    x = b.ring(P["cin"], 0, c["rate"])
    b.ring_write(x, 0)
    cr = b.ring(P["cm"], 0, c["rate"])
    op_a = b.conv("a", x, cr, fuse_next=True)
    ch = c["cout"]
    o = b.ring(ch, c["out_hist"], c["rate"] * c["up"])
    act = {None: native.ACT_NONE, "ELU": native.ACT_ELU, "LeakyReLU": native.ACT_LEAKY}[c["act"]] if act2 is None else act2
    op_b = b.conv("b", cr, o, act, c["slope"], native.ACT_TANH if c["act_out"] == "tanh" else native.ACT_NONE)
    out = b.ring(ch, 0, c["rate"] * c["up"], external=1)
    b.mean([o], out)                                                 # one source: a copy (x / 1)
    assert op_a.impl == native.IMPL_SPLIT16 and op_b.impl == (native.IMPL_SPLIT16 if ou else native.IMPL_AUTO)
    assert op_a.chain == 0 and op_b.fuse_next == 0
    if not fused:
        op_a.fuse_next = 0
    return program.HipProgram(b, c["B"], c["F"], device), cr


def run_program(pr, cr, c, xs, device="cuda:0"):
    """The call protocol on a program: per call (output (B, ch, T up), live history rows of c (B, cm, hist), flag word), on the CPU."""
    cls, _ = CC.stream_classes(c["B"])
    hk = PAIRS[c["pair"]]["hist"]
    assert pr.ring_meta[cr]["hist"] == hk
    res = []
    for (f, zero_last, reset), x in zip(CC.protocol(c), xs):
        if reset:
            pr.reset()
        if zero_last:
            pr.restore_stream_state(c["B"] - 1, None)
        T = f * c["rate"]
        xin = x[cls].transpose(1, 2).contiguous().to(device)
        y = torch.full((c["B"], T * c["up"], c["cout"]), float("nan"), device=device)
        pr.step(f, (xin, y))
        rows = (pr.cursors()[cr] - hk + torch.arange(hk, device=device)) % pr.ring_meta[cr]["rows"]
        res.append((y.transpose(1, 2).cpu(), pr._ring_view(cr)[:, rows].transpose(1, 2).cpu(), pr.flags()))
    return res


def op_names(pr, frames):
    return [pr.describe_op(i, frames) for i in range(pr.n_ops)]


KERNEL = {"ou": "conv_ou16<192>", "oc": "conv_oc16<96>"}


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
def _table():
    t = []

    def add(pair, name, B, frames, **kw):
        t.append(case(pair, name, B, frames, seed=len(t), **kw))

    # ---- ou: per MT2 two (up, cout_real) pairs; the T ladder under each activation arm; every bias combination ----
    for mt2, (pa, pb) in {1: ((2, 16), (8, 4)), 2: ((4, 16), (2, 32)), 3: ((3, 32), (8, 12))}.items():
        a, b_ = dict(up=pa[0], cout=pa[1]), dict(up=pb[0], cout=pb[1])
        add("ou", f"ou MT2 {mt2} {pa} ladder LeakyReLU 0.5 signed", 2, OU_LADDER, **a)
        add("ou", f"ou MT2 {mt2} {pb} ladder no activation signed, no bias 1", 3, OU_LADDER, act=None, b1=False, **b_)
        add("ou", f"ou MT2 {mt2} {pa} ladder ELU two-level W1, no bias 2", 2, OU_LADDER, act="ELU", kind="w1two", b2=False, **a)
        add("ou", f"ou MT2 {mt2} {pb} LeakyReLU two-level x, no biases", 2, SHORT, kind="xtwo", b1=False, b2=False, **b_)
        add("ou", f"ou MT2 {mt2} {pa} LeakyReLU 0.25 signed", 1, SHORT, slope=0.25, **a)
        add("ou", f"ou MT2 {mt2} {pb} ELU two-level W2", 5, SHORT, act="ELU", kind="w2two", **b_)
    add("ou", "ou (24, 4) ladder LeakyReLU 0.5 signed", 2, OU_LADDER, up=24, cout=4)
    add("ou", "ou (16, 4) no activation two-level W2", 2, SHORT, up=16, cout=4, act=None, kind="w2two")
    add("ou", "ou (3, 32) out ring 1 + 300 rows: phases straddle the wrap", 2, [100, 100, 37, 100, 100, 1, 100], up=3, cout=32, out_hist=1)
    add("ou", "ou (8, 4) out ring 2 + 264 rows, two-level x", 3, SHORT, up=8, cout=4, out_hist=2, kind="xtwo", act="ELU")
    add("ou", "ou (6, 16) rate 5: T 40, 15, 5", 3, [8, 8, 3, 8, 1, 8, 8], rate=5, up=6, cout=16, slope=0.25)
    add("ou", "ou (3, 32) 257 streams", 257, [17, 17, 5, 17, 1, 17, 16], up=3, cout=32)
    add("ou", "ou (2, 16) 300 streams two-level W1", 300, [16, 3, 16, 1, 16, 15], up=2, cout=16, kind="w1two")
    # ---- oc ----
    add("oc", "oc ladder A LeakyReLU 0.5 signed", 2, OC_LADDER_A)
    add("oc", "oc ladder B LeakyReLU 0.5 signed", 3, OC_LADDER_B)
    add("oc", "oc ladder B no activation signed, no bias 1", 1, OC_LADDER_B, act=None, b1=False)
    add("oc", "oc ladder A ELU two-level W1, no output bias", 2, OC_LADDER_A, act="ELU", kind="w1two", b2=False)
    add("oc", "oc ladder B LeakyReLU two-level x", 2, OC_LADDER_B, kind="xtwo")
    add("oc", "oc ladder A LeakyReLU 0.25 signed, no biases", 3, OC_LADDER_A, slope=0.25, b1=False, b2=False)
    add("oc", "oc ladder B ELU two-level x", 5, OC_LADDER_B, act="ELU", kind="xtwo")
    add("oc", "oc 257 streams x 3 slices = 771 workgroups", 257, [1] * 6, rate=366)
    add("oc", "oc rate 61: T 122, 183, 61, 366", 2, [2, 3, 1, 6, 2, 1, 6], rate=61, kind="w1two")
    return t


CASES = _table()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# act_out tanh: the operands of a case of the table, whose pre-activation form must have passed first
TANH_OF = ["oc ladder A LeakyReLU 0.5 signed", "oc ladder B LeakyReLU two-level x", "oc ladder B no activation signed, no bias 1"]


def tanh_case(name):
    return dict(CASE_BY_NAME[name], act_out="tanh", name=name + " + tanh")


# ------------------------------------------------------------------------------------------------
# the third outcome of op_pair_kind: the fused residual unit (conv_rl16_unit<32 | 64>), as one-unit chain_cases programs
# ------------------------------------------------------------------------------------------------
def unit_items(C, d, B, T):
    """Work items of the fused residual unit's workgroup for a call -- (m-tiles) x (pairs of 32-step n-tiles of its time tile), restated from
    rl16_time_tile / launch_conv_rl16_fused -- or None below 24 steps (the rows kernel is not preferred).  <= 4: four waves; 5: five; more:
    the launch declines and the unit runs as two launches."""
    if T < 24:
        return None
    tt = ((54000 // (4 * C + 16) - 6 * d) // 32) * 32
    nt32 = -(-T // 32)
    mt = C // 32
    if tt >= T:
        tt = T
    if nt32 > 1 and B * nt32 <= 768:
        tt = 32
    elif tt >= T and nt32 >= 8:
        tt = (nt32 + 1) // 2 * 32
    elif tt >= T and nt32 >= 4 and mt * ((nt32 + 1) // 2) > 4 and mt * (((nt32 + 1) // 2 + 1) // 2) <= 4:
        tt = (nt32 + 1) // 2 * 32
    return mt * ((-(-min(tt, T) // 32) + 1) // 2)


def _unit_case(name, C, B, rate, F_, d, kind, seed, frames=None):
    """A chain_cases case of ONE unit (K7 dilation d, then 1x1 + residual): two-level on non-negative data under ELU, or signed under
    LeakyReLU 0.5."""
    c = CC.case(name, 0, C, "ELU", B, rate, F_, dils=(d,), kind="twolevel", two=seed % 2, frames=frames, seed=300 + seed)
    if kind == "signed":
        c.update(act="LeakyReLU", slope=0.5, kind="signed", two=None, fan=3, xmax=1000)
    return c


UNIT_LADDER = [97, 24, 33, 64, 31, 65, 23, 97]            # n-tile edges; 23: below the rows kernel's threshold, the unit runs op by op
UNIT_CASES = [
    _unit_case("unit 32 one item per workgroup, T ladder, signed", 32, 2, 1, 97, 1, "signed", 0, UNIT_LADDER),
    _unit_case("unit 64 two items, T ladder, two-level", 64, 3, 1, 97, 3, "twolevel", 1, UNIT_LADDER),
    _unit_case("unit 64 two items, T ladder, signed", 64, 1, 1, 97, 1, "signed", 2, UNIT_LADDER),
    _unit_case("unit 32 three items of a 160-step tile, 80 streams, T 300", 32, 80, 300, 1, 1, "twolevel", 3, [1] * 6),
    _unit_case("unit 32 five items: five waves, 80 streams, dilation 9, T 330 = 320 + 10", 32, 80, 330, 1, 9, "signed", 4, [1] * 6),
    _unit_case("unit 64 four items of a 96-step tile, 130 streams, T 192", 64, 130, 192, 1, 1, "signed", 5, [1] * 6),
    _unit_case("unit 64 six items: declined, 130 streams, T 200", 64, 130, 200, 1, 1, "twolevel", 6, [1] * 6),
    _unit_case("unit 32 six items: declined, 80 streams, dilation 3, T 360", 32, 80, 360, 1, 3, "signed", 7, [1] * 6),
]
UNIT_BY_NAME = {c["name"]: c for c in UNIT_CASES}
