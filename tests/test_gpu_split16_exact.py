"""The split-f16 conv kernels bit for bit against an exact model, and the format's edges against derived bounds.

Part B.  Operands on the two-level grid of tests/split16_model.py (n + m 2^-14, lo halves non-zero) make every partial sum of the kernels'
arithmetic exactly representable in f32, whatever the summation order: each family -- conv_sk16 in its three tile configurations, conv_gv16,
conv_rk16, conv_rl16, conv_up16 -- must be torch.equal to the model computed in f64 on the CPU.  Every case asserts the model's
preconditions (operands equal to their split, S under the cap, model representable) BEFORE a kernel is called, the kernel's name, and that no
device flag was raised; it makes several calls of differing step counts so that the ring wraps, and zeroes one stream's ring and history
half-way.  tests/test_split16_model.py proves on the CPU that this comparison rejects the wrong kernels one can think of.  The exact-f32 kernels
(the guard's repair path) run the same cases on the integer grid and must equal the f64 conv.

Part C.  What the grid cannot reach: the split's rounding of lo (a set of ties), magnitudes down to 2^-40 (the f16 subnormal band: an
absolute floor of 2^-36, not a ratio to f32), ELU's negative side through the split staging, and the f16 range boundary per family
(65519.996 is carried, 65520.0 raises device flag bit 3).

The fused-tail kernels (conv_ou16, conv_oc16) have their own exact model through two convs and their own cases: tests/fused_cases.py,
tests/test_fused_cases.py, tests/test_gpu_fused_exact.py (docs/design/fused_tails.md).
(The residual-chain kernels, conv_rb16, have their own exact model and cases: tests/chain_cases.py, tests/test_gpu_chain_variants.py.)"""
import numpy as np
import pytest
import torch

import split16_model as M
from test_gpu_conv_rk16 import _eligible, _rep_class

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = [5, 7, 5, 1, 3, 5]
SK = {0: "conv_sk16<128x64>", 2: "conv_sk16<64x64>", 4: "conv_sk16<32x128>"}
RK, GV, UP = "conv_sk16<rk16 64x64>", "conv_gv16<32>", "conv_up16<64>"
FILL = 0.3                       # mean S aimed at, as a share of the cap 2^23 q: the largest S of a case then stays under it with room (asserted)


@pytest.fixture
def opts():
    """The library's process-wide options and forced tile configuration, put back whatever the test did."""
    from audiodec_amd import native
    yield native
    native.set_option("gv16_max_columns", 32)
    native.set_option("conv_rk16", 1)
    native.check(native.lib().adk_set_conv_cfg(-1), "adk_set_conv_cfg")


def _configure(native, gv=0, rk=0, cfg=-1):
    native.set_option("gv16_max_columns", gv)
    native.set_option("conv_rk16", rk)
    native.check(native.lib().adk_set_conv_cfg(cfg), "adk_set_conv_cfg")


def case(cin_g, cout_g, k, B, steps=STEPS, groups=1, rep=False, stride=1, dil=1, act=None, slope=0.0, bias=True, res=False, tr=0, pairs=False):
    """A conv case.  tr = s: the transposed conv cin_g -> cout_g, kernel 2 s, stride s (k is 2 taps of the polyphase form)."""
    return dict(cin_g=cin_g, cout_g=cout_g, k=k, B=B, steps=list(steps), groups=groups, rep=rep, stride=stride, dil=dil, act=act, slope=slope,
                bias=bias, res=res, tr=tr, pairs=pairs)


def _paired(g, shape, nmax, density, mmax):
    """Grid values whose channels (axis 1) come in pairs (2 i, 2 i + 1): the same |n|, `sign` times n, and a different m."""
    half = list(shape)
    half[1] //= 2
    base = M.grid(g, half, nmax, density, mmax).double()
    n = base.round()
    m = ((base - n) / M.UNIT).round()
    m2 = (m + 3 + torch.randint(1, 7, half, generator=g).double()) % 7 - 3
    return n, m, m2


def _operands(c, mmax):
    """Weights, bias and the calls' inputs, residuals and models -- CPU only; the model's preconditions are asserted in here."""
    g = torch.Generator().manual_seed(c["cin_g"] * 131 + c["cout_g"] * 17 + c["k"] * 7 + c["B"] + c["groups"] + c["stride"] + c["dil"] + c["tr"])
    cin_g, cout_g, groups, k, B, s, act, slope = (c[n] for n in ("cin_g", "cout_g", "groups", "k", "B", "stride", "act", "slope"))
    cin, cout = cin_g * groups, cout_g * groups
    mean_a = {None: 2.5, "ELU": 2.5, "LeakyReLU": 1.25 * (1 + slope)}[act]
    K = 2 * cin_g if c["tr"] else cin_g * k
    density = min(1.0, (FILL * 2.0 ** 23 * M.grid_unit(act, slope) - 10.0) / (K * mean_a * 2.0))       # (10: bias and residual)
    if c["tr"]:
        w = M.grid(g, (cin, cout, 2 * c["tr"]), 3, 1.0, mmax)
    elif c["pairs"]:
        n, m, m2 = _paired(g, (cout, cin_g, k), 3, 1.0, mmax)
        w = torch.stack([n + m * M.UNIT, n + m2 * M.UNIT], 2).reshape(cout, cin_g, k).float()
    else:
        w = M.grid(g, (cout, cin_g, k), 3, 1.0, mmax)
    bias = M.grid(g, (cout,), 4, 1.0, mmax) if c["bias"] else None
    span = 1 if c["tr"] else (k - 1) * c["dil"]
    hist = torch.zeros(B, cin, span)
    calls = []
    for call, t in enumerate(c["steps"]):
        reset = call == len(c["steps"]) // 2                 # one stream starts over: reset_buffer for that stream
        if reset:
            hist[B - 1] = 0
        if c["pairs"]:
            n, m, m2 = _paired(g, (B, cin, t * s), 4, density, mmax)
            x = torch.stack([n + m * M.UNIT, (-n + m2 * M.UNIT) * (n != 0)], 2).reshape(B, cin, t * s).float()
        else:
            x = M.grid(g, (B, cin, t * s), 4, density, mmax, signed=act != "ELU")
        r = M.grid(g, (B, cout, t), 4, 1.0, mmax) if c["res"] else None
        win = torch.cat([hist, x], 2)
        if c["tr"]:
            model, true, S = M.model_convtr(win, w, bias, c["tr"], act, slope)
        else:
            model, true, S = M.model_conv(win[:, :cin_g] if c["rep"] else win, w, bias, r, k, s, c["dil"], groups, act, slope, rep=c["rep"])
        if c["pairs"]:                                       # the hi*hi sum cancels: the whole output is cross terms
            assert float(model.abs().max()) < 0.25 and float((model != 0).float().mean()) > 0.9
        hist = win[:, :, win.shape[2] - span:]
        calls.append((t, reset, x, r, model, true, S))
    return w, bias, calls


def _layer(c, w, bias, impl):
    from audiodec_amd import layers
    cin, cout = c["cin_g"] * c["groups"], c["cout_g"] * c["groups"]
    if c["tr"]:
        m = layers.CausalConvTranspose1d(cin, cout, 2 * c["tr"], c["tr"], bias is not None, device=DEV, batch=c["B"], max_len=max(c["steps"])).load(w, bias)
    else:
        cls = _rep_class() if c["rep"] else layers.CausalConv1d
        m = cls(cin, cout, c["k"], c["stride"], c["dil"], c["groups"], bias is not None, device=DEV, batch=c["B"],
                max_len=max(c["steps"]) * c["stride"]).load(w, bias)
    m.set_activation(c["act"], c["slope"])
    m.impl = impl
    return m


def _poison(shape):
    """NaN-filled blocks of the output's size, freed: the layer allocates its output itself (torch.empty), and the caching allocator hands
    it -- and the copies the layer makes before it -- these blocks back (best effort: measured, most but not all of the time)."""
    blocks = [torch.full(shape, float("nan"), device=DEV) for _ in range(3)]
    del blocks


def _same(y, ref, ctx):
    y = y.cpu()
    if y.dtype != ref.dtype:
        y = y.to(ref.dtype)
    if torch.equal(y, ref):
        return
    bad = ~(y == ref)
    first = [int(i) for i in bad.nonzero()[0]]
    raise AssertionError(f"{ctx}: {int(bad.sum())} of {bad.numel()} outputs differ from the model, max |diff| "
                         f"{float((y.double() - ref.double()).abs().nan_to_num(float('inf')).max()):.3e}, first at {first}: {float(y[tuple(first)])!r} != {float(ref[tuple(first)])!r}")


def _run(native, c, impl, want, mmax=3, against_f64=False):
    w, bias, calls = _operands(c, mmax)
    m = _layer(c, w, bias, impl)
    names = set()
    for call, (t, reset, x, r, model, true, S) in enumerate(calls):
        if reset:
            m.ring[c["B"] - 1].zero_()
        _poison(tuple(model.transpose(1, 2).shape))
        y = m.inference(x.to(DEV)) if c["tr"] else m.inference(x.to(DEV), None if r is None else r.to(DEV))
        name = want(t) if callable(want) else want
        assert m.last_kernel.startswith(name) if name.endswith("<") else m.last_kernel == name, (call, t, m.last_kernel, name)
        names.add(m.last_kernel)
        _same(y, true if against_f64 else model, (c, call, t, m.last_kernel))
    assert native.device_flags() == 0
    return names


# ------------------------------------------------------------------------------------------------
# B. exact equality, family by family
# ------------------------------------------------------------------------------------------------
L64, L128 = [63, 65, 64, 1, 65], [127, 129, 128, 2, 129]          # one short of a column tile, one over, exactly one
LEAKY2, LEAKY4 = dict(act="LeakyReLU", slope=0.5), dict(act="LeakyReLU", slope=0.25)
SK_CASES = {
    # 64 x 64 tiles
    "cfg2 columns 63/64/65, ktot 96": (2, case(32, 64, 3, 1, L64, bias=True, res=True)),
    "cfg2 groups 3, ktot 224": (2, case(32, 64, 7, 3, groups=3, bias=False, res=True, **LEAKY2)),
    "cfg2 groups 3 x.repeat": (2, case(32, 64, 7, 3, groups=3, rep=True, **LEAKY4)),
    "cfg2 K 1792 dilation 9: five workgroups fold one tile": (2, case(256, 64, 7, 2, dil=9, act="ELU", bias=True, res=True)),
    "cfg2 k 10 stride 5": (2, case(32, 64, 10, 3, stride=5, bias=False)),
    "cfg2 k 4 stride 2": (2, case(32, 128, 4, 13, stride=2, res=True, **LEAKY2)),
    # 128 x 64 tiles
    "cfg0 columns 63/64/65, ktot 96": (0, case(32, 128, 3, 1, L64, bias=False)),
    "cfg0 groups 3, K 448": (0, case(64, 128, 7, 3, groups=3, res=True, **LEAKY4)),
    "cfg0 K 2816: several workgroups per tile": (0, case(256, 128, 11, 2, res=True, **LEAKY2)),
    "cfg0 groups 3 x.repeat": (0, case(32, 128, 7, 2, groups=3, rep=True)),
    "cfg0 k 10 stride 5": (0, case(32, 128, 10, 2, stride=5, bias=False)),
    # 32 x 128 tiles
    "cfg4 columns 127/128/129, cout_g 36": (4, case(32, 36, 3, 1, L128, res=True)),
    "cfg4 cout_g 96 groups 3 x.repeat": (4, case(32, 96, 7, 3, groups=3, rep=True, bias=False, **LEAKY2)),
    "cfg4 cout_g 96 groups 3": (4, case(32, 96, 3, 27, groups=3, res=True, act="ELU")),
    "cfg4 cout_g 36 k 7 dilation 9": (4, case(64, 36, 7, 2, dil=9, **LEAKY4)),
    "cfg4 k 10 stride 5": (4, case(64, 96, 10, 2, stride=5, res=True)),
}


@pytest.mark.parametrize("name", list(SK_CASES))
def test_stream_k_kernels_equal_the_model(gpu, opts, name):
    """conv_sk16 in the tile configuration named (forced only where the heuristic could pick it: 128-row tiles with cout_g % 128 == 0,
    64-row tiles with cout_g % 64 == 0)."""
    cfg, c = SK_CASES[name]
    assert cfg == 4 or c["cout_g"] % (128 if cfg == 0 else 64) == 0
    _configure(opts, gv=0, rk=0, cfg=cfg)
    _run(opts, c, opts.IMPL_SPLIT16_SK, SK[cfg])


GV_CASES = {
    "112 steps (slices of 12), columns 1/31/32": (32, case(256, 64, 7, 1, [1, 31, 32, 5, 31], res=True, **LEAKY2)),
    "224 steps (slices of 24)": (32, case(512, 32, 7, 2, bias=False)),
    "6 steps: one slice, no exchange": (32, case(32, 32, 3, 3, groups=3, res=True, **LEAKY4)),
    "three m-tiles, dilation 2": (32, case(160, 96, 3, 4, dil=2, act="ELU")),
    "k 10 stride 5": (32, case(64, 64, 10, 3, stride=5, **LEAKY2)),
    "x.repeat, groups 3": (32, case(64, 64, 11, 2, groups=3, rep=True, res=True)),
    "33 columns: a ragged second n-tile": (256, case(128, 64, 7, 3, [11, 12, 11, 1, 11], res=True, **LEAKY2)),
    "transposed, stride 5": (32, case(128, 32, 2, 2, tr=5, **LEAKY2)),
    "transposed, stride 3": (32, case(64, 32, 2, 3, tr=3, **LEAKY4)),
}


@pytest.mark.parametrize("name", list(GV_CASES))
def test_few_column_kernel_equals_the_model(gpu, opts, name):
    gv, c = GV_CASES[name]
    _configure(opts, gv=gv, rk=0)
    _run(opts, c, opts.IMPL_SPLIT16_SK, GV)


@pytest.mark.parametrize("c", [
    case(128, 64, 7, 13, act="ELU"),                                         # 65 columns: one column in the last tile
    case(128, 64, 11, 27, groups=3, rep=True, res=True, **LEAKY2),         # three n-tiles, x.repeat
    case(256, 64, 7, 1, res=True, **LEAKY4),                                # one stream: a single tile of 5 / 7 / 3 columns
], ids=["13 streams", "27 streams x.repeat", "1 stream"])
def test_rows_once_kernel_equals_the_model(gpu, opts, c):
    """conv_rk16 on the calls it takes, the stream-K kernel on those it declines (one step: no shared row; three steps at K 11: LDS), both
    continuing from the ring the other left."""
    _configure(opts, gv=0, rk=2)
    names = _run(opts, c, opts.IMPL_SPLIT16_SK, lambda t: RK if _eligible(t, c["k"], 1, c["B"]) else SK[2])
    assert names == {RK, SK[2]}, names


T24 = [23, 25, 24, 1, 40]                                                    # around the 24-step threshold of the AUTO choice; 40: a second, ragged time tile
ROWS_CASES = {
    "32 ch k 3": case(32, 32, 3, 2, T24, res=True, **LEAKY2),
    "32 ch k 7 dilation 9 groups 3": case(32, 64, 7, 2, T24, groups=3, dil=9, act="ELU"),
    "32 ch k 11": case(32, 96, 11, 3, T24, bias=False, **LEAKY4),
    "64 ch k 3 dilation 3": case(64, 64, 3, 2, T24, dil=3, res=True),
    "64 ch k 7": case(64, 32, 7, 3, T24, **LEAKY2),
    "64 ch k 11 groups 2": case(64, 64, 11, 2, T24, groups=2, res=True, **LEAKY4),
    "32 ch transposed stride 2": case(32, 16, 2, 2, T24, tr=2, **LEAKY2),
    "64 ch transposed stride 3": case(64, 32, 2, 2, T24, tr=3),
}


@pytest.mark.parametrize("name", list(ROWS_CASES))
def test_rows_in_lds_kernel_equals_the_model(gpu, opts, name):
    c = ROWS_CASES[name]
    _run(opts, c, opts.IMPL_SPLIT16_ROWS, f"conv_rl16<{c['cin_g']}>")


UP_CASES = {"32 GEMM rows": case(64, 16, 2, 2, [130, 5, 129, 1, 128], tr=2, **LEAKY2), "96 GEMM rows": case(64, 32, 2, 2, [130, 5, 129, 1, 128], tr=3)}


@pytest.mark.parametrize("name", list(UP_CASES))
def test_upsampling_streamer_equals_the_model(gpu, opts, name):
    """conv_up16 over calls whose 128-step chunks end inside a call (130 = 128 + 2) and whose history row comes from the call before."""
    _run(opts, UP_CASES[name], opts.IMPL_SPLIT16_UP, UP)


@pytest.mark.parametrize("kernel", ["sk16", "gv16"])
def test_total_cancellation_at_k_2816(gpu, opts, kernel):
    """cin_g 256, k 11: channels in pairs with negated n and another m, weights in pairs with the same n and another m -- the hi*hi sum of every
    output is exactly 0 and the whole result is cross terms (asserted on the model): near-total cancellation with one right answer."""
    if kernel == "sk16":
        _configure(opts, gv=0, rk=0)
        _run(opts, case(256, 64, 11, 2, [17, 20, 18, 1, 19], bias=False, pairs=True), opts.IMPL_SPLIT16_SK, SK[2])
    else:
        _configure(opts, gv=32, rk=0)
        _run(opts, case(256, 64, 11, 2, bias=False, pairs=True), opts.IMPL_SPLIT16_SK, GV)


TWINS = {**{n: c for n, (_, c) in SK_CASES.items()}, **{"gv16 " + n: c for n, (_, c) in GV_CASES.items()},
         **{"rl16 " + n: c for n, c in ROWS_CASES.items()}, **{"up16 " + n: c for n, c in UP_CASES.items()}}


@pytest.mark.parametrize("name", list(TWINS))
def test_exact_f32_kernels_equal_the_f64_conv_on_integers(gpu, opts, name):
    """The guard's repair path: the scalar kernel, the f32 stream-K kernel and (where it takes the shape) the f32 rows-in-LDS kernel on the
    cases above with m = 0 -- integers, halves and quarters, every partial sum exact -- must equal the f64 conv."""
    c = TWINS[name]
    _run(opts, c, opts.IMPL_DIRECT, "conv_direct", mmax=0, against_f64=True)
    _run(opts, c, opts.IMPL_MFMA, "conv_sk<", mmax=0, against_f64=True)
    if c["stride"] == 1 and c["cin_g"] in (32, 64) and c["cout_g"] % 32 == 0 and c["k"] in (3, 7, 11) and not c["rep"] and not c["tr"]:
        _run(opts, dict(c, steps=[25, 24, 40, 24]), opts.IMPL_MFMA_ROWS, "conv_rl<", mmax=0, against_f64=True)     # it takes calls of >= 24 steps


# ---- shadow ring ----
def _program(shadow, B, wa, wb, bias_b):
    """ring write -> conv a (128 -> 128, K 7, no activation) -> conv b (128 -> 128, K 11, LeakyReLU 0.5) -> out, as _two_conv_program of
    test_gpu_conv_rk16.py: lowered with shadow rings, conv a's epilogue writes the pre-activated, pre-split operands conv b stages."""
    from audiodec_amd import arch, program
    from audiodec_amd.native import ACT_LEAKY, ACT_NONE
    C = 128
    specs = [arch.ConvSpec("a", "conv", C, C, 7), arch.ConvSpec("b", "conv", C, C, 11)]
    sd = {specs[0].wkey("weight"): wa, specs[0].wkey("bias"): torch.zeros(C), specs[1].wkey("weight"): wb, specs[1].wkey("bias"): bias_b}
    old = program.SHADOW_RINGS
    program.SHADOW_RINGS = shadow
    try:
        b = program.Builder(sd, specs, split16=True)
        rx = b.ring(C, 0, 1)
        b.ring_write(rx, 0)
        mid = b.ring(C, 0, 1)
        b.conv("a", rx, mid, ACT_NONE, 0.0)
        out = b.ring(C, 0, 1, external=1)
        b.conv("b", mid, out, ACT_LEAKY, 0.5)
        pr = program.HipProgram(b, B, max(STEPS), DEV)
    finally:
        program.SHADOW_RINGS = old
    return pr


@pytest.mark.parametrize("rk", [2, 0], ids=["conv_rk16", "stream-K"])
def test_shadow_ring_operands_equal_the_model(gpu, opts, rk):
    """Conv a is a signed permutation with a one-step delay and zero bias: its output is the grid input moved around, exactly.  Conv b then
    stages what conv a's epilogue split (shadow) or splits conv a's f32 rows itself (no shadow): both must equal the model of conv b."""
    _configure(opts, gv=0, rk=rk)
    B, C = 13, 128
    g = torch.Generator().manual_seed(21)
    perm = torch.randperm(C, generator=g)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    wa = torch.zeros(C, C, 7)
    wa[torch.arange(C), perm, 5] = sign                     # tap 5 of 7: the step before the current one
    wb = M.grid(g, (C, C, 11), 3)
    bias_b = M.grid(g, (C,), 4)
    density = (FILL * 2.0 ** 23 * M.grid_unit("LeakyReLU", 0.5) - 10.0) / (C * 11 * 1.875 * 2.0)
    sh, pl = _program(True, B, wa, wb, bias_b), _program(False, B, wa, wb, bias_b)
    assert sum(1 for i in range(sh.n_ops) if sh._ops[i].in_shadow) == 1 and sum(1 for i in range(sh.n_ops) if sh._ops[i].out_shadow) == 1
    assert not any(pl._ops[i].in_shadow or pl._ops[i].out_shadow for i in range(pl.n_ops))
    last = torch.zeros(B, C, 1)                              # the input step before this call
    hist = torch.zeros(B, C, 10)                             # conv b's history: conv a's last ten outputs
    for call, t in enumerate(STEPS):
        if call == 3:
            last[B - 1] = 0
            hist[B - 1] = 0
            for pr in (sh, pl):
                pr.restore_stream_state(B - 1, None)
        x = M.grid(g, (B, C, t), 4, density)
        xa = torch.cat([last, x], 2)
        mid = xa[:, perm, :t] * sign.view(1, C, 1)           # conv a, exactly
        win = torch.cat([hist, mid], 2)
        model, _, _ = M.model_conv(win, wb, bias_b, None, 11, 1, 1, 1, "LeakyReLU", 0.5)
        last, hist = xa[:, :, t:], win[:, :, t:]
        for pr in (sh, pl):
            names = [pr.describe_op(i, t) for i in range(pr.n_ops)]
            assert names[1] == (RK if rk and _eligible(t, 7, 1, B) else SK[2]) and names[2] == (RK if rk and _eligible(t, 11, 1, B) else SK[2]), (t, names)
            y = torch.full((B, t, C), float("nan"), device=DEV)
            pr.step(t, (x.transpose(1, 2).contiguous().to(DEV), y))
            _same(y.transpose(1, 2), model, ("shadow" if pr is sh else "no shadow", call, t))
    assert sh.flags() == 0 and pl.flags() == 0 and opts.device_flags() == 0


# ------------------------------------------------------------------------------------------------
# C. the format's edges
# ------------------------------------------------------------------------------------------------
# family -> (options, impl name, channels, columns, kernel name): identity / permutation 1x1 convs, one stream
ONE_BY_ONE = {
    "sk16 128x64": (dict(gv=0, rk=0, cfg=0), "IMPL_SPLIT16_SK", 128, 65, SK[0]),
    "sk16 64x64": (dict(gv=0, rk=0, cfg=2), "IMPL_SPLIT16_SK", 128, 65, SK[2]),
    "sk16 32x128": (dict(gv=0, rk=0, cfg=4), "IMPL_SPLIT16_SK", 128, 129, SK[4]),
    "gv16": (dict(gv=32, rk=0), "IMPL_SPLIT16_SK", 128, 31, GV),
    "rl16<32>": (dict(), "IMPL_SPLIT16_ROWS", 32, 40, "conv_rl16<32>"),
    "rl16<64>": (dict(), "IMPL_SPLIT16_ROWS", 64, 40, "conv_rl16<64>"),
}


def _one_by_one(native, family, w, x, act=None):
    from audiodec_amd import layers
    o, impl, C, L, name = ONE_BY_ONE[family]
    _configure(native, **o)
    m = layers.CausalConv1d(C, C, 1, 1, 1, 1, False, device=DEV, batch=1, max_len=x.shape[2]).load(w, None)
    m.set_activation(act, 0.0)
    m.impl = getattr(native, impl)
    _poison((1, x.shape[2], C))
    y = m.inference(x.to(DEV)).cpu()
    assert m.last_kernel == name, (family, m.last_kernel)
    return y


@pytest.mark.parametrize("family", list(ONE_BY_ONE))
def test_the_split_rounds_lo_to_nearest_even(gpu, opts, family):
    """split16_model.rounding_set through a signed permutation: every lo half is a tie, the answer hi + lo / 2048 is exact -- a split that
    truncates lo, or rounds ties away, is off by 2^-22 on three quarters / a quarter of the outputs."""
    C, L = ONE_BY_ONE[family][2:4]
    g = torch.Generator().manual_seed(31)
    perm = torch.randperm(C, generator=g)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    w = torch.zeros(C, C, 1)
    w[torch.arange(C), perm, 0] = sign
    x = M.rounding_set(g, (1, C, L))
    y = _one_by_one(opts, family, w, x)
    _same(y, M.joined(x)[:, perm] * sign.view(1, C, 1), family)
    assert opts.device_flags() == 0


def _small_values(g, n):
    """|v| log-uniform over [2^-40, 2^-10], both signs, after the exact powers of two 2^-40 ... 2^-10 (2^-20 is entry 20)."""
    v = torch.cat([2.0 ** torch.arange(-40, -9).double(), 2.0 ** (torch.rand(n - 31, generator=g).double() * 30 - 40)])
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    s[:31] = 1
    return (v * s).float()


@pytest.mark.parametrize("family", list(ONE_BY_ONE))
def test_small_magnitudes_keep_an_absolute_floor(gpu, opts, family):
    """An identity 1x1 conv (weights exact 1 and 0, lo = 0) returns hi + lo / 2048 of each activation.  For an f16-normal hi the rounding of
    lo leaves at most 2^-22 |v|; in the f16 subnormal band (|v| < 2^-14, or (v - hi) * 2048 there) the quantum of lo is 2^-24, which after
    / 2048 leaves at most 2^-36 (half a quantum, 2^-25, of hi's rounding is carried by lo; lo's own half quantum is 2^-25 / 2048); the join
    rounds once more (2^-24 |v|).  So |y - v| <= 1.25 2^-22 |v| + 2^-36: an absolute floor -- relative to f32 the format is far worse down
    there by construction.  And 2^-20 comes back as 2^-20, not as 0: the matrix cores honour f16 subnormal inputs."""
    C, L = ONE_BY_ONE[family][2:4]
    g = torch.Generator().manual_seed(41)
    x = _small_values(g, C * L).view(1, L, C).transpose(1, 2).contiguous()
    y = _one_by_one(opts, family, torch.eye(C).unsqueeze(-1), x)
    err = (y.double() - x.double()).abs()
    bound = 1.25 * 2.0 ** -22 * x.double().abs() + 2.0 ** -36
    worst = float((err / bound).max())
    sub = x.abs() < 2.0 ** -14
    print(f"{family}: max err / bound {worst:.3f}; subnormal band: {int((y[sub] == 0).sum())} of {int(sub.sum())} outputs are 0, "
          f"max |err| there {float(err[sub].max()):.3e} (2^-36 = {2.0 ** -36:.3e}); f(2^-20) = {float(y[0, 20 % C, 20 // C])!r}")
    assert float(x[0, 20 % C, 20 // C]) == 2.0 ** -20 and float(y[0, 20 % C, 20 // C]) != 0.0, "an activation of 2^-20 came back as 0"
    assert bool((err <= bound).all()), (family, worst)
    assert opts.device_flags() == 0


@pytest.mark.parametrize("family", ["sk16 32x128", "rl16<32>"])
def test_elu_negative_side_through_the_split_staging(gpu, opts, family):
    """The input set of test_elu_of_the_kernels_against_fp64 (tests/test_gpu_parity.py) through identity 1x1 convs on the split-f16
    kernels: 4e-7 is that test's bound for expm1_neg, 2^-21 |ref| + 2^-36 is the format (above, rounded up)."""
    C, L = 32, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.cat([-torch.logspace(-7, 1.3, C * L // 2, dtype=torch.float64), torch.rand(C * L // 2, generator=g, dtype=torch.float64) * 3 - 1])
    x = x[torch.randperm(C * L, generator=g)].float().view(1, C, L)
    ref = torch.nn.functional.elu(x.double())
    from audiodec_amd import layers
    _configure(opts, gv=0, rk=0)
    m = layers.CausalConv1d(C, C, 1, 1, 1, 1, False, device=DEV, batch=1, max_len=L).load(torch.eye(C).unsqueeze(-1), None)
    m.set_activation("ELU", 0.0)
    m.impl = opts.IMPL_SPLIT16_SK if family.startswith("sk16") else opts.IMPL_SPLIT16_ROWS
    y = m.inference(x.to(DEV)).cpu().double()
    assert m.last_kernel == ("conv_sk16<32x128>" if family.startswith("sk16") else "conv_rl16<32>"), m.last_kernel
    err, bound = (y - ref).abs(), (4e-7 + 2.0 ** -21) * ref.abs() + 2.0 ** -36
    print(f"{family}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert opts.device_flags() == 0


BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))            # 65519.996: f16 rounds it to 65504
# family -> (options, impl, case, kernel, P): the column count leaves a ragged last tile; P = most partial sums a tile is added from (stream-K:
# kMaxSplit workgroups, conv_gv16: 24 steps in slices of 12)
EDGE = {
    "sk16 128x64": (dict(gv=0, rk=0, cfg=0), "IMPL_SPLIT16_SK", case(128, 128, 3, 1, [70]), SK[0], 5),
    "sk16 64x64": (dict(gv=0, rk=0, cfg=2), "IMPL_SPLIT16_SK", case(128, 128, 3, 1, [70]), SK[2], 5),
    "sk16 32x128": (dict(gv=0, rk=0, cfg=4), "IMPL_SPLIT16_SK", case(128, 36, 3, 1, [134]), SK[4], 5),
    "gv16": (dict(gv=256, rk=0), "IMPL_SPLIT16_SK", case(128, 64, 3, 1, [38]), GV, 2),
    "rk16": (dict(gv=0, rk=2), "IMPL_SPLIT16_SK", case(128, 64, 7, 14, [5]), RK, 1),
    "rl16<32>": (dict(), "IMPL_SPLIT16_ROWS", case(32, 32, 3, 2, [38]), "conv_rl16<32>", 1),
    "rl16<64>": (dict(), "IMPL_SPLIT16_ROWS", case(64, 64, 7, 2, [38]), "conv_rl16<64>", 1),
    "up16": (dict(), "IMPL_SPLIT16_UP", case(64, 16, 2, 2, [134], tr=2), UP, 1),
}


@pytest.mark.parametrize("family", list(EDGE))
def test_range_boundary(gpu, opts, family):
    """65519.996 (the f32 below 65520) is the largest magnitude f16 rounds to 65504: planted among grid operands -- in the first and the last
    input channel (the first and last row of the staged operand tile), at the last step, a column of the ragged last tile -- it raises no flag.
    Its split is hi = 65504, lo = 32768 (15.996 * 2048 = 32760 is a tie between 32752 and 32768): off by 2^-8, a relative 2^-24.  Every product
    and every sum inside the two accumulators is still exact (integers below 2^24, eighths below 2^21).  What rounds, by at most 2^-24 of a
    value no larger than S = sum |a| |w| + |bias| + |res|: the joins of the P partial sums a tile is added from (their S add up to S: 2^-24 S
    together), the P - 1 additions of those, the bias add and the residual add.  So |y - model| <= (P + 2) 2^-24 S with the model of
    split16_model in f64 (P <= 5); against the true conv the planted operand's representation error (2^-24) and the dropped lo*lo term
    (<= 2^-22 S) come on top, and the issue's |y - f64| <= 2^-21 S is asserted as well.
    65520.0 itself, at each of the three places in turn, rounds to inf in f16: device flag bit 3, sticky until read, then clear."""
    o, impl, c, name, P = EDGE[family]
    _configure(opts, **o)
    w, bias, calls = _operands(c, 3)
    t, _, x, r, _, _, _ = calls[0]
    m = _layer(c, w, bias, getattr(opts, impl))
    cin = c["cin_g"] * c["groups"]
    last = x.shape[2] - 1
    spots = [(c["B"] - 1, 0, last), (c["B"] - 1, cin - 1, last), (0, cin // 2, 0)]

    def run(xp):
        m.reset_buffer()
        y = m.inference(xp.to(DEV)) if c["tr"] else m.inference(xp.to(DEV), None if r is None else r.to(DEV))
        assert m.last_kernel == name, (family, m.last_kernel)
        return y.cpu()

    xp = x.clone()
    xp[spots[0]], xp[spots[1]], xp[spots[2]] = BELOW, -BELOW, -BELOW
    y = run(xp)
    assert opts.device_flags() == 0, "65519.996 raised a flag"
    win = torch.cat([torch.zeros(c["B"], cin, 1 if c["tr"] else (c["k"] - 1) * c["dil"]), xp], 2)
    if c["tr"]:
        model, true, S = M.unchecked_convtr(win, w, bias, c["tr"], None, 0.0)
    else:
        model, true, S = M.unchecked_conv(win, w, bias, r, c["k"], 1, c["dil"], 1, None, 0.0)
    assert float(S.max()) > 65504.0
    e_model, e_true = (y.double() - model).abs() / S, (y.double() - true).abs() / S
    print(f"{family}: max |y - model| / S = {float(e_model.max()):.3e} ({P + 2} * 2^-24 = {(P + 2) * 2.0 ** -24:.3e}), max |y - f64| / S = {float(e_true.max()):.3e} (2^-21 = {2.0 ** -21:.3e})")
    assert bool((e_model <= (P + 2) * 2.0 ** -24).all()) and bool((e_true <= 2.0 ** -21).all()), (family, float(e_model.max()), float(e_true.max()))
    for i, spot in enumerate(spots):
        xp = x.clone()
        xp[spot] = 65520.0 if i != 1 else -65520.0
        run(xp)
        assert opts.device_flags() & 8, (family, spot, "65520 raised no flag")
        assert opts.device_flags() == 0, "the flag is cleared by the read"
