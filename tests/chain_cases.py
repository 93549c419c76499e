"""Residual-chain mini-programs, an exact model of a whole chain, and an f32 emulation that can be made wrong on purpose.

Plain helper for tests/test_chain_cases.py (CPU) and tests/test_gpu_chain_variants.py (GPU); importing it needs no GPU.

THE PROGRAM.  program.Builder with a synthetic state dict and hand-made arch.ConvSpecs: a ring write from ext[0], ONE residual chain of
n_units units (conv A: ta taps, dilation d_u; conv B: tb taps, dilation 1; + the unit's input), and an output ring.  The chain program marks
the chain (op.chain = 2 n_units, every op IMPL_SPLIT16: csrc/conv_rb16.hip takes it where adk_conv_rb16_plan says so); the per-op program has
chain = 0, fuse_next = 0 and, at 32 / 64 channels, every op forced to IMPL_SPLIT16_ROWS -- the rows-in-LDS kernel tests/test_gpu_split16_exact.py
pins bit for bit, whose operation order the chain claims to reproduce.  T = steps per frame (`rate`) x frames of the call.

THE EXACT MODEL.  The argument of tests/split16_model.py carried through a chain.  Node k (the input of conv k, raw) lies on a grid of unit
u_k; its activated form on qa_k = u_k (ELU on non-negative data, LeakyReLU on non-negative data: the identity) or u_k * slope (a power of
two); the weights of conv k on qw_k = 1 (integers) or 2^-14 (two-level, n + m 2^-14: lo != 0).  hi and lo / 2048 of an operand are multiples
of its unit, so every product of the three MFMA sums is a multiple of q_k = qa_k qw_k, and with

    S_k = sum |a| |w| + |bias| + |residual|  <  2^23 q_k

every partial sum in any order, the join, the bias add and the residual add (bias an integer, the residual on the coarser grid u_{k-1}) are
exact in f32.  The kernel must then be torch.equal to the f64 chain, each conv minus its dropped lo*lo term (split16_model.evaluate), and its
output is on the grid u_{k+1} = q_k.  The budget: a LeakyReLU on signed data costs log2(1 / slope) bits per conv, two-level weights 14 bits
from that conv on.  So the cases are of two kinds:
  * `signed`: integer weights (+-1, a few per output row), integer inputs of magnitude up to 1000, slope 0.5 (three units) or 0.25 (two):
    node magnitudes pass 2^11 units, so the lo half of the activations is live from the second conv on (asserted);
  * `twolevel` at conv j: everything non-negative (inputs, weights, biases: ELU and LeakyReLU are then the identity and cost nothing), conv j
    carries `fan2` two-level weights per output row, the others one integer weight per row; from conv j on the nodes carry 2^-14 fractions
    (lo live) under a cap of 512.  Between them the cases put the two-level conv at every position of the chain.
run_model ASSERTS, before any kernel is called: operands equal to their split, S_k under the cap, every node representable and on its grid
(split16_model.combine), ELU nodes >= 0, >= 90 % of every call's outputs and of every node's stored history rows (those written since the rings were last zeroed) non-zero.

THE CALL PROTOCOL (shared by every GPU case): >= 6 calls of mixed frame counts (the ring cursors wrap every call: rows = history + one full
step), the last stream's rings zeroed half-way (restore_stream_state), one whole-program reset.  After every call the output, every ring's live
history rows and the program's flag word are compared.

Streams: a launch needs hundreds of streams to reach some arms; the model would not.  Stream b carries the input of class b % 5, the last
stream (the one that is zeroed) a class of its own: the model is computed per class and expanded."""
import functools

import torch
import torch.nn.functional as F

import split16_model as M

ACT_ELU, ACT_LEAKY = 1, 2
TAPSETS = {"K11": (11, 11, "LeakyReLU"), "K7": (7, 7, "LeakyReLU"), "K3": (3, 3, "LeakyReLU"), "ELU": (7, 1, "ELU")}
ARMS = {1: "32 ring", 2: "32 few two tiles", 3: "32 three tiles K11", 4: "32 three tiles", 5: "32 four tiles", 6: "64 ring", 7: "64 few two tiles",
        8: "64 three tiles", 9: "64 four tiles", 10: "128 one stream one tile", 11: "128 two tiles", 12: "128 two streams one tile"}
ARM_SMAX = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 2, 9: 2, 10: 1, 11: 2, 12: 2}      # streams the arm's history staging is sized for
MAX_HIST = 56
CLASSES = 5


def case(name, arm, C, tapset, B, rate, F_, groups=1, dils=(1, 3, 5), kind="signed", slope=0.5, two=None, fan=None, fan2=8, xmax=None,
         bias=True, rep=False, ext_last=False, frames=None, seed=0):
    """One chain case.  arm: what adk_conv_rb16_plan must report for a full step (rate * F_ steps); kind: 'signed' | 'twolevel' (two = position
    of the two-level conv); frames: the call protocol (default below)."""
    ta, tb, act = TAPSETS[tapset]
    if kind == "twolevel":
        assert two is not None and 0 <= two < 2 * len(dils)
    else:
        assert act != "ELU", "ELU stays exact only on non-negative data"
    if frames is None:
        short = max(1, F_ // 3)
        frames = [F_, F_, short, F_, F_, 1, F_] if F_ > 1 else [1] * 6
    return dict(name=name, arm=arm, C=C, tapset=tapset, ta=ta, tb=tb, act=act, B=B, rate=rate, F=F_, groups=groups, dils=tuple(dils), kind=kind,
                slope=slope if act == "LeakyReLU" else 0.0, two=two, fan=fan if fan is not None else (3 if kind == "signed" and slope == 0.5 else (2 if kind == "signed" else 1)),
                fan2=fan2, xmax=xmax if xmax is not None else (1000 if kind == "signed" else 3), bias=bias, rep=rep, ext_last=ext_last,
                frames=list(frames), seed=seed)


def n_convs(c):
    return 2 * len(c["dils"])


def conv_geometry(c, k):
    """(taps, dilation, history rows) of conv k."""
    taps = c["tb"] if k & 1 else c["ta"]
    dil = 1 if k & 1 else c["dils"][k // 2]
    return taps, dil, (taps - 1) * dil


def plan_dilations(c):
    return [conv_geometry(c, k)[1] for k in range(n_convs(c))]


def plan(c, frames=None, native=None):
    """adk_conv_rb16_plan for a call of `frames` frames (default: a full step)."""
    if native is None:
        from audiodec_amd import native
    return native.conv_rb16_plan(c["C"], c["ta"], c["tb"], ACT_ELU if c["act"] == "ELU" else ACT_LEAKY, plan_dilations(c), c["B"], c["groups"],
                                 c["rate"] * (c["F"] if frames is None else frames))


def stream_classes(B):
    """(class of every stream, number of classes): b % CLASSES, and a class of its own for the last stream (the one the protocol zeroes)."""
    d = min(B, CLASSES)
    cls = [b % d for b in range(B)]
    if B > 1:
        cls[B - 1] = d
        return torch.tensor(cls), d + 1
    return torch.tensor(cls), 1


def protocol(c):
    """[(frames, zero the last stream's rings first, reset the whole program first)] of the case's calls."""
    n = len(c["frames"])
    return [(f, i == n // 2, i == n - 2) for i, f in enumerate(c["frames"])]


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def _sparse_rows(g, rows, cols, fan):
    """(rows, fan) distinct column indices per row."""
    return torch.rand(rows, cols, generator=g).argsort(1)[:, :fan]


@functools.lru_cache(maxsize=None)
def _operands_cached(key):
    c = dict(key)
    g = torch.Generator().manual_seed(1000 + c["seed"])
    C, G = c["C"], c["groups"]
    ws, bs = [], []
    for k in range(n_convs(c)):
        taps = conv_geometry(c, k)[0]
        two = c["kind"] == "twolevel" and c["two"] == k
        fan = min(c["fan2"] if two else c["fan"], C * taps)
        idx = _sparse_rows(g, C * G, C * taps, fan)
        if c["kind"] == "signed":
            v = (torch.randint(0, 2, idx.shape, generator=g) * 2 - 1).double()
        else:
            v = torch.ones(idx.shape, dtype=torch.float64)
            if two:
                v = torch.randint(1, 3, idx.shape, generator=g).double()
                m = torch.randint(1, 4, idx.shape, generator=g).double() * (torch.randint(0, 2, idx.shape, generator=g) * 2 - 1).double()
                v = v + m * M.UNIT
        w = torch.zeros(C * G, C * taps, dtype=torch.float64)
        w.scatter_(1, idx, v)
        ws.append(w.view(C * G, C, taps).float())
        if c["bias"]:
            b = torch.randint(1, 5, (C * G,), generator=g).float()
            if c["kind"] == "signed":
                b = b * (torch.randint(0, 2, (C * G,), generator=g) * 2 - 1).float()
        else:
            b = None
        bs.append(b)
    _, ncls = stream_classes(c["B"])
    cin = C if c["rep"] else C * G
    xs = []
    for f, _, _ in protocol(c):
        x = torch.randint(1, c["xmax"] + 1, (ncls, cin, f * c["rate"]), generator=g).float()
        if c["kind"] == "signed":
            x = x * (torch.randint(0, 2, x.shape, generator=g) * 2 - 1).float()
        xs.append(x)
    return ws, bs, xs


def _key(c):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in c.items()))


def operands(c):
    """(weights [(C G, C, taps)], biases, per-call inputs [(classes, cin, T)]) of an exact case."""
    return _operands_cached(_key(c))


def real_operands(c):
    """Gaussian weights, biases and inputs of both signs for the case's shape (the bit-identity runs): no model, ELU's negative side live."""
    g = torch.Generator().manual_seed(5000 + c["seed"])
    C, G = c["C"], c["groups"]
    ws, bs = [], []
    for k in range(n_convs(c)):
        taps = conv_geometry(c, k)[0]
        ws.append(torch.randn(C * G, C, taps, generator=g) * (0.7 / (C * taps) ** 0.5))
        bs.append(torch.randn(C * G, generator=g) * 0.1 if c["bias"] else None)
    _, ncls = stream_classes(c["B"])
    cin = C if c["rep"] else C * G
    xs = [torch.randn(ncls, cin, f * c["rate"], generator=g) for f, _, _ in protocol(c)]
    return ws, bs, xs


# ------------------------------------------------------------------------------------------------
# the exact model
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_cached(key):
    c = dict(key)
    ws, bs, xs = _operands_cached(key)
    n, G, C = n_convs(c), c["groups"], c["C"]
    _, ncls = stream_classes(c["B"])
    cin = C if c["rep"] else C * G
    hist = [torch.zeros(ncls, cin if k == 0 else C * G, conv_geometry(c, k)[2], dtype=torch.float64) for k in range(n)]
    calls, share, lo_act, lo_w = [], 0.0, [[] for _ in range(n)], [float((M.split(w)[1] != 0).float().mean()) for w in ws]
    stored, stored_nz = [0] * n, [0] * n
    filled = [0] * ncls                                  # steps a class has taken since its rings were last zeroed
    for (f, zero_last, reset), x in zip(protocol(c), xs):
        if reset:
            for h in hist:
                h.zero_()
            filled = [0] * ncls
        if zero_last:
            for h in hist:
                h[ncls - 1] = 0
            filled[ncls - 1] = 0
        filled = [v + f * c["rate"] for v in filled]
        nodes, unit = [x.double()], 1.0
        for k in range(n):
            taps, dil, hk = conv_geometry(c, k)
            win = torch.cat([hist[k], nodes[k]], 2)
            nonneg = bool((win >= 0).all())
            assert c["act"] != "ELU" or nonneg, f"{c['name']}: conv {k} has a negative ELU input"
            qa = unit if (c["act"] == "ELU" or nonneg) else unit * c["slope"]
            assert bool(((win / unit).round() * unit == win).all()), f"{c['name']}: node {k} is off its grid"
            qw = M.UNIT if (c["kind"] == "twolevel" and c["two"] == k) else 1.0
            q = qa * qw
            rep = G if (c["rep"] and k == 0) else 0
            p = M.parts(win, ws[k], c["act"], c["slope"], rep)
            res = None
            if k & 1:
                res = nodes[k - 1].repeat(1, G, 1) if (c["rep"] and k == 1) else nodes[k - 1]
            conv = (lambda d: (lambda a_, w_: F.conv1d(a_, w_, None, 1, 0, d, G)))(dil)
            model, _, smax = M.combine(conv, *p, bs[k], res, q)
            share = max(share, smax / (2.0 ** 23 * q))
            lo_act[k].append(float((p[2] != 0).double().mean()))
            nodes.append(model.double())
            unit = q
            if hk:
                hist[k] = win[:, :, win.shape[2] - hk:].clone()
                for cl in range(ncls):                   # (rows older than the last zeroing are zero by construction: not counted)
                    part = hist[k][cl, :, hk - min(hk, filled[cl]):]
                    stored[k] += part.numel()
                    stored_nz[k] += int((part != 0).sum())
        out = nodes[n].float()
        assert float((out != 0).float().mean()) >= 0.9, f"{c['name']}: a call's outputs are mostly zero"
        calls.append(dict(frames=f, zero_last=zero_last, reset=reset, x=x, out=out, hist=[h.float() for h in hist]))
    for k in range(1, n):
        assert stored[k] == 0 or stored_nz[k] >= 0.9 * stored[k], f"{c['name']}: the stored history of node {k} is mostly zero"
    lo_act = [sum(v) / len(v) for v in lo_act]
    if c["kind"] == "signed":
        assert all(v >= 0.05 for v in lo_act[1:]), f"{c['name']}: the lo half of the activations is not live from the second conv on: {lo_act}"
    else:
        assert lo_w[c["two"]] > 0 and all(v == 0 for k, v in enumerate(lo_w) if k != c["two"])
        assert all(v >= 0.25 for v in lo_act[c["two"] + 1:]), f"{c['name']}: the nodes behind the two-level conv carry no lo half: {lo_act}"
    return calls, dict(share=share, lo_act=lo_act, lo_w=lo_w)


def run_model(c):
    """(calls, stats): per call the inputs, the model's output (classes, C G, T) and the live history rows of every node (classes, ch, hist_k)
    after it; stats: the largest S as a share of its cap, the share of activations / weights with a live lo half per conv."""
    return _model_cached(_key(c))


# ------------------------------------------------------------------------------------------------
# f32 emulation of the chain over explicit rings, right or wrong
# ------------------------------------------------------------------------------------------------
FAULTS = ["hist_shift", "no_wrap", "res_prev", "keep_less", "cut_1024", "drop_wlo_ahi", "drop_alo_whi", "swap_columns", "bias_before_join"]


def _act32(v, act, slope):
    if act == "ELU":
        return F.elu(v)
    return torch.where(v > 0, v, v * slope)


def emulate(c, ws, bs, xs, fault=None, at=1, shuffle=True):
    """The chain in f32 as conv_rb16 runs it -- rings with cursors, history fetched in front of the new rows, of an intermediate node only the
    rows later calls need stored, three sums per conv joined as m + c / 2048, then bias, then residual -- summed in chunks of a SHUFFLED k
    order (shuffle=False: taps ascending, channels ascending, the kernels' order).  Streams are the case's classes, two per workgroup where
    the arm takes two.  fault: one of FAULTS, applied to conv `at` where it names one conv.  Returns per call (output, [live history rows])."""
    n, G, C = n_convs(c), c["groups"], c["C"]
    _, ncls = stream_classes(c["B"])
    cin = C if c["rep"] else C * G
    g = torch.Generator().manual_seed(77)
    step = c["rate"] * c["F"]
    geo = [conv_geometry(c, k) for k in range(n)]
    rows = [geo[k][2] + step for k in range(n)]
    rings = [torch.zeros(ncls, rows[k], cin if k == 0 else C * G) for k in range(n)]
    cur = [0] * n
    spw = 2 if c["arm"] in (11, 12) and c["B"] * G > 128 else 1
    out = []
    for (f, zero_last, reset), x in zip(protocol(c), xs):
        T = f * c["rate"]
        if reset:
            for r in rings:
                r.zero_()
            cur = [0] * n
        if zero_last:
            for k in range(n):
                rings[k][ncls - 1, (cur[k] - geo[k][2] + torch.arange(geo[k][2])) % rows[k]] = 0
        new = [x.float().transpose(1, 2).contiguous()]                     # node k's new rows, (classes, T, ch)
        rings[0][:, (cur[0] + torch.arange(T)) % rows[0]] = new[0]
        for k in range(n):
            taps, dil, hk = geo[k]
            ch = rings[k].shape[2]
            ridx = cur[k] - hk + torch.arange(hk)
            if fault == "hist_shift" and k == at:
                ridx = ridx - 1
            if fault == "no_wrap" and k >= 1:
                flat = torch.arange(ncls)[:, None] * rows[k] + ridx[None, :]          # below row 0: the end of the stream in front
                h = rings[k].reshape(-1, ch)[flat.clamp(min=0)] * (flat >= 0)[:, :, None]
            else:
                h = rings[k][:, ridx % rows[k]]
            if fault == "cut_1024" and spw == 2 and k >= 1 and hk:
                piece = hk * (C // 8) + torch.arange(hk)[:, None] * (C // 8) + torch.arange(C // 8)[None, :]      # the second stream's pieces
                keep = (piece < 1024).repeat_interleave(8, 1).repeat(1, G)                                         # (hk, ch), every group alike
                h = h.clone()
                h[1::2] = h[1::2] * keep[None]
            a = _act32(torch.cat([h, new[k]], 1).transpose(1, 2), c["act"], c["slope"])
            if c["rep"] and k == 0:
                a = a.repeat(1, G, 1)
            ah, al = (t.float() for t in M.split(a))
            wh, wl = (t.float().view(G, C, C * taps) for t in M.split(ws[k]))          # [g][row][c * taps + tap]
            sel = (torch.arange(T)[None, :] + (torch.arange(taps) * dil)[:, None])          # (taps, T) window columns
            ch_, cl_ = (t.view(ncls, G, C, hk + T)[:, :, :, sel].reshape(ncls, G, C * taps, T) for t in (ah, al))
            kk = C * taps
            order = torch.randperm(kk, generator=g) if shuffle else torch.arange(kk).view(C, taps).t().reshape(-1)
            m = torch.zeros(ncls, G, C, T)
            cc = torch.zeros(ncls, G, C, T)
            chunk = 16 if kk <= 512 else 64
            for i in range(0, kk, chunk):
                j = order[i:i + chunk]
                m = m + torch.einsum("goj,bgjt->bgot", wh[:, :, j], ch_[:, :, j])
                if not (fault == "drop_alo_whi" and k == at):
                    cc = cc + torch.einsum("goj,bgjt->bgot", wh[:, :, j], cl_[:, :, j])
                if not (fault == "drop_wlo_ahi" and k == at):
                    cc = cc + torch.einsum("goj,bgjt->bgot", wl[:, :, j], ch_[:, :, j])
            b = bs[k].view(1, G, C, 1) if bs[k] is not None else None
            if fault == "bias_before_join" and b is not None:
                y = (m + b) + cc * (1.0 / 2048.0)
            else:
                y = m + cc * (1.0 / 2048.0)
                if b is not None:
                    y = y + b
            y = y.reshape(ncls, G * C, T).transpose(1, 2)                  # (classes, T, ch)
            if k & 1:
                src = k - 3 if (fault == "res_prev" and k >= 3) else k - 1
                r = new[src]
                y = y + (r.repeat(1, 1, G) if r.shape[2] != G * C else r)
            if fault == "swap_columns" and spw == 2 and T % 32 and k == n - 1:
                t0 = T // 32 * 32
                cnt = min(T - t0, 32 - (T - t0), T)
                y = y.clone()
                for s in range(0, ncls - 1, 2):
                    first, second = y[s, t0:t0 + cnt].clone(), y[s + 1, :cnt].clone()
                    y[s, t0:t0 + cnt], y[s + 1, :cnt] = second, first
            new.append(y.contiguous())
            if k + 1 < n:
                keep_rows = T if k & 1 else min(T, geo[k + 1][2] - (1 if fault == "keep_less" else 0))
                t = torch.arange(T - keep_rows, T)
                rings[k + 1][:, (cur[k + 1] + t) % rows[k + 1]] = y[:, t]
        for k in range(n):
            cur[k] = (cur[k] + T) % rows[k]
        out.append((new[n].transpose(1, 2).contiguous(),
                    [rings[k][:, (cur[k] - geo[k][2] + torch.arange(geo[k][2])) % rows[k]].transpose(1, 2).contiguous() for k in range(n)]))
    return out


# ------------------------------------------------------------------------------------------------
# the programs (GPU)
# ------------------------------------------------------------------------------------------------
def build_program(c, ws, bs, chain, device="cuda:0", unit=False):
    """(HipProgram, ring of every node 0 .. n): the chain program (chain=True) or its per-op twin.  unit=True: no chain, every op left to
    the runner's own choice (IMPL_SPLIT16) and every unit's first conv marked fuse_next -- the fused residual unit, conv_rl16_unit<C>
    (tests/test_gpu_fused_exact.py)."""
    from audiodec_amd import arch, native, program
    n, G, C = n_convs(c), c["groups"], c["C"]
    act = ACT_ELU if c["act"] == "ELU" else ACT_LEAKY
    specs, sd = [], {}
    for k in range(n):
        taps, dil, _ = conv_geometry(c, k)
        s = arch.ConvSpec(f"u{k // 2}.{'b' if k & 1 else 'a'}", "conv", C * G, C * G, taps, 1, dil, G, bs[k] is not None)
        specs.append(s)
        sd[s.wkey("weight")] = ws[k]
        if bs[k] is not None:
            sd[s.wkey("bias")] = bs[k]
    b = program.Builder(sd, specs, split16=True)
    x = b.ring(C if c["rep"] else C * G, 0, c["rate"])
    b.ring_write(x, 0)
    node_rings, ops = [x], []
    for u in range(n // 2):
        first = c["rep"] and u == 0                                  # x.repeat(1, groups, 1) never materialised: group stride 0
        xt = b.ring(C * G, 0, c["rate"])
        ops.append(b.conv(specs[2 * u].name, x, xt, act, c["slope"], in_group_stride=0 if first else None))
        last = u == n // 2 - 1
        nx = b.ring(C * G, 0, c["rate"], external=1 if (last and c["ext_last"]) else -1)
        ops.append(b.conv(specs[2 * u + 1].name, xt, nx, act, c["slope"], res_ring=x, res_group_stride=0 if first else None))
        node_rings += [xt, nx]
        x = nx
    if not c["ext_last"]:
        out = b.ring(C * G, 0, c["rate"], external=1)
        b.mean([x], out)                                             # one source: a copy (x / 1)
    for op in ops:
        assert op.impl == native.IMPL_SPLIT16
        op.chain, op.fuse_next = 0, 0
        if not chain and not unit and C in (32, 64):
            op.impl = native.IMPL_SPLIT16_ROWS
    if unit:
        assert not chain
        for op in ops[0::2]:
            op.fuse_next = 1
    if chain:
        ops[0].chain = n
    return program.HipProgram(b, c["B"], c["F"], device), node_rings


def run_program(pr, node_rings, c, xs, device="cuda:0"):
    """The call protocol on a program: per call (output (B, C G, T), [live history rows of node k (B, ch, hist_k)], flag word), on the CPU."""
    cls, _ = stream_classes(c["B"])
    n = n_convs(c)
    res = []
    for (f, zero_last, reset), x in zip(protocol(c), xs):
        if reset:
            pr.reset()
        if zero_last:
            pr.restore_stream_state(c["B"] - 1, None)
        T = f * c["rate"]
        xin = x[cls].transpose(1, 2).contiguous().to(device)
        y = torch.full((c["B"], T, c["C"] * c["groups"]), float("nan"), device=device)
        pr.step(f, (xin, y))
        cur = pr.cursors()
        hist = []
        for k in range(n):
            r, hk = node_rings[k], conv_geometry(c, k)[2]
            assert pr.ring_meta[r]["hist"] == hk
            rows = (cur[r] - hk + torch.arange(hk, device=device)) % pr.ring_meta[r]["rows"]
            hist.append(pr._ring_view(r)[:, rows].transpose(1, 2).cpu())
        res.append((y.transpose(1, 2).cpu(), hist, pr.flags()))
    return res


def chain_op_names(pr, frames):
    return [pr.describe_op(i, frames) for i in range(pr.n_ops)]


# ------------------------------------------------------------------------------------------------
# the case table: every reachable (arm, tap set) pair
# ------------------------------------------------------------------------------------------------
def _table():
    t = []
    pos = {True: 0, False: 0}                            # the next position of the two-level conv, ELU and LeakyReLU cases apart

    def add(name, arm, C, tapset, B, rate, F_, **kw):
        """Kinds in turn: ELU cases are two-level (non-negative); LeakyReLU cases alternate signed slope 0.5 / two-level / signed slope 0.25."""
        i = len(t)
        dils = kw.pop("dils", (1, 3, 9) if tapset == "ELU" else (1, 3, 5))
        kind = kw.pop("kind", "twolevel" if tapset == "ELU" else ("signed", "twolevel", "signed4")[i % 3])
        if kind == "twolevel":
            elu = tapset == "ELU"
            two = kw.pop("two", pos[elu] % (2 * len(dils)))
            pos[elu] += 1
            kw.setdefault("fan2", 8 if two < 4 else 5)           # (the nodes have grown by the third unit: fewer two-level weights per row fit the cap)
            t.append(case(name, arm, C, tapset, B, rate, F_, dils=dils, kind="twolevel", two=two, seed=i, **kw))
        elif kind == "signed4":
            t.append(case(name, arm, C, tapset, B, rate, F_, dils=dils[:2], kind="signed", slope=0.25, seed=i, **kw))
        else:
            t.append(case(name, arm, C, tapset, B, rate, F_, dils=dils, kind="signed", slope=0.5, seed=i, **kw))

    # ---- 32 channels ----
    add("32 ring K11, 129 workgroups (warm-up on), T 40 and 25", 1, 32, "K11", 43, 5, 8, groups=3, frames=[8, 8, 5, 8, 8, 1, 8])
    add("32 ring K7, 387 workgroups (warm-up off)", 1, 32, "K7", 129, 5, 5, groups=3)
    add("32 ring K3, 270 workgroups (tile rotation)", 1, 32, "K3", 90, 11, 3, groups=3)
    add("32 ring ELU, 130 workgroups, T 100", 1, 32, "ELU", 130, 25, 4, bias=False)
    add("32 few K11, 1 workgroup", 2, 32, "K11", 1, 5, 8)
    add("32 few K7, 9 workgroups", 2, 32, "K7", 3, 13, 3, groups=3)
    add("32 few K3, 64 workgroups", 2, 32, "K3", 64, 7, 5)
    add("32 few ELU, 65 workgroups (no helpers)", 2, 32, "ELU", 65, 25, 2)
    add("32 three tiles K11 (late residual), T 258", 3, 32, "K11", 2, 43, 6)
    add("32 three tiles K7, T 384", 4, 32, "K7", 3, 128, 3)
    add("32 three tiles K3, T 257", 4, 32, "K3", 2, 257, 1, frames=[1] * 6)
    add("32 three tiles ELU, T 300", 4, 32, "ELU", 2, 100, 3, bias=False)
    add("32 four tiles K11, T 512 (LDS over 64 KiB)", 5, 32, "K11", 2, 128, 4)
    add("32 four tiles K7, T 385", 5, 32, "K7", 1, 77, 5)
    add("32 four tiles K3, T 387, three groups", 5, 32, "K3", 2, 129, 3, groups=3)
    add("32 four tiles ELU, T 500", 5, 32, "ELU", 2, 100, 5)
    # ---- 64 channels ----
    add("64 ring K11, 129 workgroups, T 40", 6, 64, "K11", 43, 5, 8, groups=3, frames=[8, 8, 5, 8, 8, 1, 8])
    add("64 ring K7, 390 workgroups, T 33", 6, 64, "K7", 130, 11, 3, groups=3)
    add("64 ring K3, 129 workgroups, T 128", 6, 64, "K3", 129, 32, 4)
    add("64 ring ELU, 257 workgroups, T 25", 6, 64, "ELU", 257, 25, 1, bias=False, frames=[1] * 6)
    add("64 few K11, 3 workgroups", 7, 64, "K11", 1, 5, 8, groups=3)
    add("64 few K7, 128 workgroups", 7, 64, "K7", 128, 5, 5)
    add("64 few K3, 10 workgroups", 7, 64, "K3", 10, 13, 5)
    add("64 few ELU, 1 workgroup, T 100", 7, 64, "ELU", 1, 25, 4)
    add("64 three tiles K11, T 129", 8, 64, "K11", 2, 43, 3)
    add("64 three tiles K7, T 192, 130 workgroups", 8, 64, "K7", 130, 64, 3)
    add("64 three tiles K3, T 150, three groups", 8, 64, "K3", 3, 50, 3, groups=3)
    add("64 three tiles ELU, T 160", 8, 64, "ELU", 2, 40, 4, bias=False)
    add("64 four tiles K11, T 193", 9, 64, "K11", 2, 193, 1, frames=[1] * 6)
    add("64 four tiles K7, T 256", 9, 64, "K7", 3, 64, 4)
    add("64 four tiles K3, T 200", 9, 64, "K3", 1, 50, 4)
    add("64 four tiles ELU, T 250, three groups", 9, 64, "ELU", 2, 50, 5, groups=3)
    # ---- 128 channels ----
    add("128 one stream K11, T 25", 10, 128, "K11", 3, 5, 5, groups=3)
    add("128 one stream K7, T 32, 128 workgroups", 10, 128, "K7", 128, 8, 4)
    add("128 one stream K3, T 1 .. 12", 10, 128, "K3", 2, 1, 12)
    add("128 one stream ELU, T 25", 10, 128, "ELU", 5, 25, 1, frames=[1] * 6)
    add("128 two tiles K11, one stream, T 33", 11, 128, "K11", 2, 11, 3)
    add("128 two tiles K7, two streams, B 43 odd x 3 groups, T 25", 11, 128, "K7", 43, 5, 5, groups=3, dils=(1, 6, 9))
    add("128 two tiles K3, one stream, T 64", 11, 128, "K3", 3, 16, 4)
    add("128 two tiles ELU, two streams, B 129 odd, T 17", 11, 128, "ELU", 129, 17, 1, frames=[1] * 6)
    add("128 two tiles K11, two streams, B 131 odd, T 32", 11, 128, "K11", 131, 8, 4, kind="twolevel")
    add("128 two streams one tile K11 dilation 4 / 5 (history 40 / 50), T 15", 12, 128, "K11", 43, 5, 3, groups=3, dils=(1, 4, 5), kind="twolevel")
    add("128 two streams one tile K7 dilation 6 / 9 (history 36 / 54), T 16", 12, 128, "K7", 129, 4, 4, dils=(1, 6, 9), kind="twolevel")
    add("128 two streams one tile K3, T 12", 12, 128, "K3", 130, 12, 1, frames=[1] * 6)
    add("128 two streams one tile ELU dilation 6 / 9 (history 36 / 54), T 12", 12, 128, "ELU", 43, 4, 3, groups=3, dils=(1, 6, 9))
    add("128 two streams one tile K11 dilation 4 / 5, signed, B 129 odd, T 5 .. 15", 12, 128, "K11", 129, 5, 3, dils=(1, 4, 5), kind="signed")
    # ---- the forms the lowerings use ----
    add("32 ring K11, x.repeat at three groups", 1, 32, "K11", 43, 5, 8, groups=3, rep=True, kind="signed")
    add("64 few K11, x.repeat at three groups, two-level first conv", 7, 64, "K11", 2, 5, 8, groups=3, rep=True, kind="twolevel", two=0)
    add("128 one stream K11, x.repeat at three groups", 10, 128, "K11", 2, 5, 5, groups=3, rep=True, kind="twolevel", two=1)
    add("64 ring K7, external last ring", 6, 64, "K7", 129, 5, 5, ext_last=True, kind="signed")
    add("32 few ELU, external last ring", 2, 32, "ELU", 4, 25, 2, ext_last=True)
    add("128 two tiles K3, external last ring", 11, 128, "K3", 2, 16, 4, ext_last=True, kind="signed")
    return t


CASES = _table()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
COVERED = {(c["arm"], c["tapset"]) for c in CASES}          # the (arm, tap set) pairs the GPU tests claim to cover
