"""The two fused vocoder-tail launches (csrc/conv_ou16.hip, csrc/conv_oc16.hip) bit for bit against an exact model, at every tile edge.

tests/fused_cases.py holds one mini-program per case -- op A (1x1 conv, fuse_next) + op B, a fused twin and a two-launch twin -- with operands
for which the arithmetic of both convs has one right answer; tests/test_fused_cases.py proves on the CPU that the model's preconditions hold,
that the table reaches the edges it claims and that the comparison rejects the wrong kernels one can think of.  Here, per case:
  * describe_op names conv_ou16<192> / conv_oc16<96> + "(fused into the previous op)" for EVERY call length of the fused twin, neither for
    the two-launch twin;
  * both twins are torch.equal to the f64 model: the output, the live RAW history rows of c (one for ou, six for oc) and the flag word after
    every call of a protocol with wrapping rings, T ladders (ou: 1, 2, 15, 16, 17, 100, 127, 128; oc: 1 .. 366 over one, two and three
    slices), a zeroed stream and a whole-program reset -- for all three MT2 arms of conv_ou16, the three ACT arms of both kernels, and every
    bias combination;
  * act_out tanh (oc): torch.equal to the two-launch twin, after the pre-activation case on the same operands has passed;
  * a call the launch declines (T = 129) runs as two launches and still equals the model; a tanh input activation is declined by the fused
    launch and is an error of the two-launch form (conv_up16 has no such arm), not a silent fall-back;
  * the format's edges (65519.996 carried, 65520.0 raises flag bit 3, the split's ties) through a one-hot W1;
  * Gaussian operands of both signs (ELU's negative side, slope 0.01 + tanh): fused against two-launch within the project's 2e-6
    (measured on an MI355X: conv_ou16 at most 9.0e-8 of the largest output, conv_oc16 0 -- bit-equal);
  * the third outcome of op_pair_kind, the fused residual unit conv_rl16_unit<32 | 64>, at one to five items and declined, against the
    chain model of tests/chain_cases.py.
64 tests, 3.5 s on an MI355X; the slowest (257 streams x 366 steps of conv_oc16) takes 0.24 s."""
import functools

import numpy as np
import pytest
import torch

import chain_cases as CC
import fused_cases as FC
import split16_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))            # 65519.996: f16 rounds it to 65504


def _same(got, want, ctx):
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    first = [int(i) for i in bad.nonzero()[0]]
    raise AssertionError(f"{ctx}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| "
                         f"{float((got.double() - want.double()).abs().nan_to_num(float('inf')).max()):.3e}, first at {first}: "
                         f"{float(got[tuple(first)])!r} != {float(want[tuple(first)])!r}")


def _check_names(c, pr_f, pr_t, declined=()):
    """Every call length of the case: the fused twin names the pair's kernel and the op fused into it, the two-launch twin neither."""
    k = FC.KERNEL[c["pair"]]
    for f in sorted(set(c["frames"])):
        nf, nt = FC.op_names(pr_f, f), FC.op_names(pr_t, f)
        assert nf[0] == "ring_write" and len(nf) == 4, nf
        if f in declined:
            assert not any("ou16" in n or "oc16" in n or "fused" in n for n in nf), (f, nf)
        else:
            assert nf[1] == k and nf[2] == "(fused into the previous op)", (f, nf)
        assert not any("ou16" in n or "oc16" in n or "fused" in n or "unit" in n for n in nt), (f, nt)


def _twins(c, ops):
    pr_f, cr = FC.build_program(c, ops, True, DEV)
    pr_t, cr_t = FC.build_program(c, ops, False, DEV)
    assert cr == cr_t and pr_f.arena_floats == pr_t.arena_floats
    return pr_f, pr_t, cr


@functools.lru_cache(maxsize=None)
def _exact(name):
    """Both twins of a table case against the model; returns the largest S share.  Cached: the tanh cases require it of their operands."""
    from audiodec_amd import native
    c = FC.CASE_BY_NAME[name]
    calls, stats = FC.run_model(c)
    ops, xs = FC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t)
    for which, pr in (("fused", pr_f), ("two launches", pr_t)):
        for i, (call, (y, hist, flags)) in enumerate(zip(calls, FC.run_program(pr, cr, c, xs, DEV))):
            ctx = (name, which, "call", i, "T", call["T"])
            assert flags == 0, ctx
            _same(y, call["out"][cls], ctx + ("output",))
            _same(hist, call["hist"][cls], ctx + ("history of c",))
    assert native.device_flags() == 0
    return stats["share"]


@pytest.mark.parametrize("name", list(FC.CASE_BY_NAME))
def test_fused_launch_equals_the_exact_model(gpu, name):
    share = _exact(name)
    print(f"{name}: largest S {100 * share:.1f} % of its cap")


@pytest.mark.parametrize("name", FC.TANH_OF)
def test_tanh_output_equals_the_two_launch_twin(gpu, name):
    """act_out tanh: both forms apply the same act_apply to a pre-activation that is bit-equal (the case without tanh, same operands, passes
    first), so they must be torch.equal; the history rows of c still equal the model."""
    from audiodec_amd import native
    _exact(name)
    c = FC.tanh_case(name)
    calls, _ = FC.run_model(c)
    ops, xs = FC.operands(c)
    ops0, xs0 = FC.operands(FC.CASE_BY_NAME[name])
    assert all(torch.equal(a, b) for a, b in zip(xs, xs0)) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ops, ops0))
    cls, _ = CC.stream_classes(c["B"])
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t)
    got_f, got_t = FC.run_program(pr_f, cr, c, xs, DEV), FC.run_program(pr_t, cr, c, xs, DEV)
    worst = 0.0
    for i, (call, (yf, hf, ff), (yt, ht, ft)) in enumerate(zip(calls, got_f, got_t)):
        ctx = (c["name"], "call", i, "T", call["T"])
        assert ff == 0 and ft == 0, ctx
        assert bool((yt.abs() <= 1).all())
        _same(yf, yt, ctx + ("output",))
        _same(hf, call["hist"][cls], ctx + ("history of c",))
        _same(ht, call["hist"][cls], ctx + ("history of c, two launches",))
        worst = max(worst, float((yf.double() - call["out"][cls].double()).abs().max()))
    print(f"{c['name']}: fused == two launches; max |y - tanh64(model)| = {worst:.2e}")
    assert native.device_flags() == 0


def test_a_declined_length_runs_as_two_launches_and_still_matches(gpu):
    """T = 129 is one step more than eight waves of 16 hold: conv_ou16_fusable declines, the program runs conv_sk16 + conv_up16 for that
    call and the fused launch for the others, each continuing from the history row the other left -- exact against the model."""
    from audiodec_amd import native
    c = FC.case("ou", "ou (3, 32) T 129 declined", 3, [129, 1, 128, 129, 16, 129, 129, 17], up=3, cout=32, seed=201)
    calls, _ = FC.run_model(c)
    ops, xs = FC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t, declined=(129,))
    assert FC.op_names(pr_f, 129)[1].startswith("conv_sk16") and FC.op_names(pr_f, 129)[2] == "conv_up16<64>", FC.op_names(pr_f, 129)
    for i, (call, (y, hist, flags)) in enumerate(zip(calls, FC.run_program(pr_f, cr, c, xs, DEV))):
        assert flags == 0
        _same(y, call["out"][cls], (c["name"], i, "T", call["T"], "output"))
        _same(hist, call["hist"][cls], (c["name"], i, "T", call["T"], "history of c"))
    assert native.device_flags() == 0


def test_a_tanh_input_activation_is_declined_not_run_wrong(gpu):
    """a2.act_in = tanh: conv_ou16 has no such arm and conv_ou16_fusable says so (describe_op names no conv_ou16); the two-launch form it
    falls to has none either (conv_up16), and says so with an error -- no launch under another activation, no silent fall-back."""
    from audiodec_amd import native
    c = FC.case("ou", "ou tanh", 2, [16, 1, 16, 2, 16, 16], up=3, cout=32, seed=202)
    ops, xs = FC.operands(c)
    pr, cr = FC.build_program(c, ops, True, DEV, act2=native.ACT_TANH)
    for f in (1, 2, 16):
        names = FC.op_names(pr, f)
        assert not any("ou16" in n or "fused" in n for n in names), names
    x = xs[0][:1].repeat(c["B"], 1, 1).transpose(1, 2).contiguous().to(DEV)
    y = torch.full((c["B"], 16 * 3, 32), float("nan"), device=DEV)
    with pytest.raises((native.NativeError, ValueError), match="activation"):
        pr.step(16, (x, y))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "op B ran although its activation has no kernel"
    pr.flags()
    native.device_flags()


# ------------------------------------------------------------------------------------------------
# the format's edges, through a one-hot W1
# ------------------------------------------------------------------------------------------------
EDGE_FRAMES = {"ou": [17, 2, 17, 16, 17, 17], "oc": [27, 6, 123, 7, 27, 123]}


def _edge_setup(pair, scale, seed):
    """A case without zeroed stream or reset in its way (both come after the planted call's effects are compared: calls 0 and 1 only count
    there), a one-hot W1 (+-scale), small signed integer x, the case's own W2 / b2."""
    c = FC.case(pair, f"{pair} edge", 3, EDGE_FRAMES[pair], up=3, cout=32, act="LeakyReLU", slope=0.5, b1=False, seed=seed)
    (_, _, w2, b2), xs = FC.operands(c)
    w1, perm, sgn = FC.one_hot_w1(c, seed, scale)
    g = torch.Generator().manual_seed(300 + seed)
    xs = [(torch.randint(1, 4, x.shape, generator=g) * (torch.randint(0, 2, x.shape, generator=g) * 2 - 1)).float() for x in xs]
    return c, (w1, None, w2, b2), xs, perm, sgn


@pytest.mark.parametrize("pair", ["ou", "oc"])
def test_65519_996_is_carried_through_the_first_conv(gpu, pair):
    """x = +-65519.996 at the last step of call 0 (first and last stream, first and last row of W1): its split is 65504 + 32768 / 2048, so
    c = +-65520.0 exactly -- no flag from GEMM 1, and the history row says so.  oc: the f32 output conv takes it (integers below 2^24:
    equal to the f64 model, flag word 0).  ou: the kernel splits act(c) again and 65520.0 (a positive c: LeakyReLU leaves it) rounds to inf
    in f16 -- the flag word must be the two-launch twin's, bit 3, in the call that computes c and in the next, whose older tap it is."""
    from audiodec_amd import native
    c, ops, xs, perm, sgn = _edge_setup(pair, 1.0, 11)
    ncls, T0 = xs[0].shape[0], xs[0].shape[2]
    xs[0][0, perm[0], T0 - 1] = BELOW * float(sgn[0])                 # c = +65520 in stream class 0, row 0
    xs[0][ncls - 1, perm[-1], T0 - 1] = BELOW * float(sgn[-1])        # ... and in the last stream, last row
    cls, _ = CC.stream_classes(c["B"])
    model = FC.unchecked_model(c, ops, xs[:2])
    assert float(model[0][1][0, 0, -1]) == 65520.0 and float(model[0][1][ncls - 1, -1, -1]) == 65520.0
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t)
    got_f, got_t = FC.run_program(pr_f, cr, c, xs, DEV), FC.run_program(pr_t, cr, c, xs, DEV)
    for i in (0, 1):
        (yf, hf, ff), (yt, ht, ft) = got_f[i], got_t[i]
        assert ff == ft, (pair, i, ff, ft)
        _same(hf, model[i][1][cls].float(), (pair, i, "history of c"))
        _same(ht, model[i][1][cls].float(), (pair, i, "history of c, two launches"))
        if pair == "oc":
            assert ff == 0, "65519.996 raised a flag"
            _same(yf, model[i][0][cls].float(), (pair, i, "output"))
        else:
            assert ff == 8, (i, ff)
            clean = torch.isfinite(yt)
            assert bool((torch.isfinite(yf) == clean).all()) and bool(clean[1].all())          # (stream 1 carries no planted value)
            _same(yf[clean], model[i][0][cls].float()[clean], (pair, i, "outputs the planted value does not feed"))
    for (yf, hf, ff), (yt, ht, ft) in zip(got_f[2:], got_t[2:]):          # the history row has moved on
        assert ff == 0 and ft == 0
        _same(yf, yt, (pair, "later calls"))
    assert native.device_flags() == 0


def test_65519_996_halved_passes_both_splits_of_conv_ou16(gpu):
    """A one-hot W1 of +-0.5: c = +-32760, finite in f16 (hi 32768, lo -16384: exact), so the second split carries it: flag word 0 and the
    output equals the f64 model (every sum an integer or a half far below 2^23)."""
    from audiodec_amd import native
    c, ops, xs, perm, sgn = _edge_setup("ou", 0.5, 12)
    ncls, T0 = xs[0].shape[0], xs[0].shape[2]
    xs[0][0, perm[0], T0 - 1] = BELOW
    xs[0][ncls - 1, perm[-1], 0] = -BELOW
    xs[0][1, perm[31], 15] = BELOW                                     # lane 15 of wave 0: the halo row of wave 1
    cls, _ = CC.stream_classes(c["B"])
    model = FC.unchecked_model(c, ops, xs[:2])
    assert float(model[0][1][0, 0, -1].abs()) == 32760.0
    pr_f, pr_t, cr = _twins(c, ops)
    for pr in (pr_f, pr_t):
        got = FC.run_program(pr, cr, c, xs, DEV)
        for i in (0, 1):
            y, h, fl = got[i]
            assert fl == 0, (i, fl)
            assert bool((model[i][0].float().double() == model[i][0]).all())
            _same(y, model[i][0][cls].float(), ("halved", i, "output"))
            _same(h, model[i][1][cls].float(), ("halved", i, "history of c"))
    assert native.device_flags() == 0


@pytest.mark.parametrize("pair", ["ou", "oc"])
def test_65520_raises_flag_bit_3(gpu, pair):
    """65520.0 itself rounds to inf in f16 in the FIRST split: bit 3 of the program's flag word, in the fused twin as in the other; read
    once, then clear; ou: the next calls (whose history row it left) give the twin's flag words too."""
    from audiodec_amd import native
    for spot in (0, 1, 2):
        c, ops, xs, perm, sgn = _edge_setup(pair, 1.0, 13 + spot)
        ncls, T0 = xs[0].shape[0], xs[0].shape[2]
        where = [(0, int(perm[0]), T0 - 1), (ncls - 1, 191 if pair == "ou" else 95, 0), (1, 0, T0 // 2)][spot]     # any input channel: hi = inf poisons the MFMA column
        xs[0][where] = 65520.0 if spot != 1 else -65520.0
        pr_f, pr_t, cr = _twins(c, ops)
        got_f, got_t = FC.run_program(pr_f, cr, c, xs, DEV), FC.run_program(pr_t, cr, c, xs, DEV)
        assert got_f[0][2] & 8 and got_t[0][2] & 8, (pair, spot, got_f[0][2], got_t[0][2])
        if pair == "ou":                                                   # (oc: the twin's f32 output conv and the fused kernel test different tensors for later calls)
            assert [g[2] for g in got_f] == [g[2] for g in got_t], (pair, spot)
        assert pr_f.flags() == 0 and pr_t.flags() == 0, "the flag is cleared by the read"
    native.device_flags()


@pytest.mark.parametrize("pair", ["ou", "oc"])
def test_the_splits_ties_through_a_one_hot_w1(gpu, pair):
    """split16_model.rounding_set through a signed one-hot W1: every lo half is a tie, c must be +-joined(x) exactly -- a split that truncates
    or rounds ties away is off by one lo ulp.  c shows in its history rows: the last row (ou) / six rows (oc) of every call, all streams."""
    from audiodec_amd import native
    c, ops, _, perm, sgn = _edge_setup(pair, 1.0, 21)
    g = torch.Generator().manual_seed(77)
    _, ncls = CC.stream_classes(c["B"])
    xs = [M.rounding_set(g, (ncls, FC.PAIRS[pair]["cin"], f)) for f in c["frames"]]
    assert not bool(M.split_exact(xs[0]).all())
    cls, _ = CC.stream_classes(c["B"])
    hk = FC.PAIRS[pair]["hist"]
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t)
    for which, pr in (("fused", pr_f), ("two launches", pr_t)):
        for i, (x, (y, h, fl)) in enumerate(zip(xs, FC.run_program(pr, cr, c, xs, DEV))):
            assert fl == 0 and x.shape[2] >= hk
            want = (M.joined(x)[:, perm] * sgn.view(1, -1, 1))[:, :, x.shape[2] - hk:]
            _same(h, want[cls], (pair, which, i, "history of c"))
            assert bool(torch.isfinite(y).all())
    assert native.device_flags() == 0


# ------------------------------------------------------------------------------------------------
# real values: what no grid reaches
# ------------------------------------------------------------------------------------------------
REAL = {
    "ou (2, 16) ELU": dict(pair="ou", up=2, cout=16, act="ELU"),
    "ou (2, 16) LeakyReLU 0.01": dict(pair="ou", up=2, cout=16, act="LeakyReLU", slope=0.01),
    "ou (4, 16) ELU": dict(pair="ou", up=4, cout=16, act="ELU"),
    "ou (2, 32) LeakyReLU 0.01": dict(pair="ou", up=2, cout=32, act="LeakyReLU", slope=0.01),
    "ou (3, 32) ELU": dict(pair="ou", up=3, cout=32, act="ELU"),
    "ou (3, 32) LeakyReLU 0.01": dict(pair="ou", up=3, cout=32, act="LeakyReLU", slope=0.01),
    "ou (24, 4) no activation": dict(pair="ou", up=24, cout=4, act=None),
    "oc LeakyReLU 0.01 + tanh": dict(pair="oc", act="LeakyReLU", slope=0.01, act_out="tanh"),
    "oc ELU": dict(pair="oc", act="ELU"),
    "oc ELU + tanh, no biases": dict(pair="oc", act="ELU", act_out="tanh", b1=False, b2=False),
}
REAL_FRAMES = {"ou": [128, 1, 128, 1, 100, 1, 128], "oc": [366, 1, 366, 1, 300, 1, 366]}


@pytest.mark.parametrize("name", list(REAL))
def test_fused_against_two_launches_on_real_values(gpu, name):
    """Gaussian weights and inputs of both signs at the ends of each pair's T ladder: ELU's negative side, slope 0.01, tanh.  The bound is the
    project's own for this comparison (tests/test_gpu_fused_ends.py, tests/test_gpu_b256.py): 2e-6, relative to the largest output, which
    is asserted to lie in (0.1, 4].  The worst value is printed; whether the raw history rows of c (the 1x1 conv: 32x32x16 MFMAs in both
    forms of oc, 16x16x32 against 32x32x16 in ou) happen to be bit-equal is printed, not required."""
    from audiodec_amd import native
    kw = dict(REAL[name])
    pair = kw.pop("pair")
    c = FC.case(pair, name, 3, REAL_FRAMES[pair], kind="xtwo", seed=list(REAL).index(name), **kw)          # (the kind is not used: real_operands)
    ops, xs = FC.real_operands(c)
    pr_f, pr_t, cr = _twins(c, ops)
    _check_names(c, pr_f, pr_t)
    got_f, got_t = FC.run_program(pr_f, cr, c, xs, DEV), FC.run_program(pr_t, cr, c, xs, DEV)
    scale = max(float(yt.abs().max()) for yt, _, _ in got_t)
    assert 0.1 < scale <= 4.0, scale
    worst = worst_h = 0.0
    for (yf, hf, ff), (yt, ht, ft) in zip(got_f, got_t):
        assert ff == 0 and ft == 0 and bool(torch.isfinite(yf).all())
        worst = max(worst, float((yf - yt).abs().max()) / scale)
        worst_h = max(worst_h, float((hf - ht).abs().max()))
    print(f"{name}: max |fused - two launches| / max |y| = {worst:.2e} (max |y| = {scale:.2f}); history rows of c "
          f"{'bit-equal' if worst_h == 0.0 else f'differ by up to {worst_h:.2e}'}")
    assert worst <= 2e-6
    assert worst_h <= 2e-6 * max(1.0, max(float(ht.abs().max()) for _, ht, _ in got_t))
    assert native.device_flags() == 0


# ------------------------------------------------------------------------------------------------
# the third outcome of op_pair_kind: the fused residual unit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FC.UNIT_BY_NAME))
def test_fused_residual_unit_equals_the_exact_model(gpu, name):
    """conv_rl16_unit<32 | 64> (K7 conv -> 1x1 conv + residual in one launch) as a one-unit chain_cases program with chain = 0, fuse_next = 1:
    one to four items on four waves, five items on five waves, time tiles of 32, 96, 160 and 320 steps with ragged ends, against the f64
    model of tests/chain_cases.py -- outputs, history rows and flag word after every call.  A call of more than five items (declined by the
    launcher at run time) or of fewer than 24 steps (declined by conv_rl16_fusable) runs as two launches, which equal the model too."""
    from audiodec_amd import native
    c = FC.UNIT_BY_NAME[name]
    calls, stats = CC.run_model(c)
    ws, bs, xs = CC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr_u, rings = CC.build_program(c, ws, bs, chain=False, device=DEV, unit=True)
    pr_o, rings_o = CC.build_program(c, ws, bs, chain=False, device=DEV)
    for f in sorted(set(c["frames"])):
        items = FC.unit_items(c["C"], c["dils"][0], c["B"], f * c["rate"])
        nu, no = CC.chain_op_names(pr_u, f), CC.chain_op_names(pr_o, f)
        if items is not None:
            # (describe_op asks conv_rl16_fusable, which does not count the items: for a call of more than five it still names the unit, and
            # launch_conv_rl16_fused then declines at run time -- tests/test_gpu_b256.py pins that name at whole-model shapes.  What such a call
            # computes is compared below.)
            assert nu[1] == f"conv_rl16_unit<{c['C']}>" and nu[2] == "(fused into the previous op)", (f, items, nu)
        else:
            assert not any("unit" in n or "fused" in n for n in nu), (f, items, nu)
        assert not any("unit" in n or "fused" in n or "rb16" in n for n in no), (f, no)
    for which, pr, rr in (("unit", pr_u, rings), ("op by op", pr_o, rings_o)):
        for i, (call, (y, hist, flags)) in enumerate(zip(calls, CC.run_program(pr, rr, c, xs, DEV))):
            ctx = (name, which, "call", i, "frames", call["frames"])
            assert flags == 0, ctx
            _same(y, call["out"][cls], ctx + ("output",))
            for k, h in enumerate(hist):
                _same(h, call["hist"][k][cls], ctx + ("history of node", k))
    assert native.device_flags() == 0
    print(f"{name}: largest S {100 * stats['share']:.1f} % of the cap")
