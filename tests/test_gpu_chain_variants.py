"""Every launch variant of the residual-chain kernel (csrc/conv_rb16.hip) against an exact model and against the per-op kernels.

launch_conv_rb16 picks one of twelve template arms (adk_conv_rb16_plan names it), each built for four tap sets.  tests/chain_cases.py holds
one mini-program per reachable (arm, tap set) pair -- tests/test_chain_cases.py proves on the CPU that the table covers exactly the pairs the
plan can reach, that the exact model's preconditions hold, and that the comparison rejects the wrong chains one can think of.  Here, per case:
  * the plan query names the arm the case is about, describe_op names conv_rb16<C> for the chain program and no rb16 for the per-op one;
  * on grid operands the chain must be torch.equal to the f64 model: the output, every ring's live history rows and the flag word after
    every call of a protocol with wrapping rings, short steps, a zeroed stream and a whole-program reset;
  * on Gaussian operands of both signs (ELU's negative side live) the 32- and 64-channel chains must be torch.equal to the per-op program on
    the rows-in-LDS kernel (tests/test_gpu_split16_exact.py pins that one), outputs and history rows, over the same protocol."""
import pytest
import torch

import chain_cases as CC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _same(got, want, ctx):
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    first = [int(i) for i in bad.nonzero()[0]]
    raise AssertionError(f"{ctx}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| "
                         f"{float((got.double() - want.double()).abs().nan_to_num(float('inf')).max()):.3e}, first at {first}: "
                         f"{float(got[tuple(first)])!r} != {float(want[tuple(first)])!r}")


def _check_names(c, pr_chain, pr_perop=None):
    """describe_op of a full step: the chain program runs conv_rb16<C> where the plan takes the call, the per-op program never."""
    names = CC.chain_op_names(pr_chain, c["F"])
    assert names[0] == "ring_write" and names[1] == f"conv_rb16<{c['C']}>", names
    assert all(n == "(fused into the previous op)" for n in names[2:1 + CC.n_convs(c)]), names
    if pr_perop is not None:
        for f in sorted(set(c["frames"])):
            names = CC.chain_op_names(pr_perop, f)
            assert not any("rb16" in n or "fused" in n or "unit" in n for n in names), names
            if c["C"] in (32, 64):
                assert names[1:1 + CC.n_convs(c)] == [f"conv_rl16<{c['C']}>"] * CC.n_convs(c), names


def _assert_plan(c, native):
    p = CC.plan(c, native=native)
    assert p["taken"] and p["arm"] == c["arm"], (c["name"], CC.ARMS[c["arm"]], p)
    return p


@pytest.mark.parametrize("name", list(CC.CASE_BY_NAME))
def test_chain_equals_the_exact_model(gpu, name):
    """The chain kernel on the case's arm, bit for bit against the f64 model (whose preconditions run_model asserts first)."""
    from audiodec_amd import native
    c = CC.CASE_BY_NAME[name]
    calls, stats = CC.run_model(c)
    _assert_plan(c, native)
    ws, bs, xs = CC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr, rings = CC.build_program(c, ws, bs, chain=True, device=DEV)
    _check_names(c, pr)
    got = CC.run_program(pr, rings, c, xs, DEV)
    for i, (call, (y, hist, flags)) in enumerate(zip(calls, got)):
        ctx = (name, "call", i, "frames", call["frames"])
        assert flags == 0, ctx
        _same(y, call["out"][cls], ctx + ("output",))
        for k, h in enumerate(hist):
            _same(h, call["hist"][k][cls], ctx + ("history of node", k))
    assert native.device_flags() == 0
    print(f"{name}: arm {c['arm']} ({CC.ARMS[c['arm']]}), largest S {100 * stats['share']:.1f} % of the cap")


def _run_pair(c, ws, bs, xs):
    """(chain program's results, per-op program's results) over the case's protocol."""
    pr_c, rings_c = CC.build_program(c, ws, bs, chain=True, device=DEV)
    pr_o, rings_o = CC.build_program(c, ws, bs, chain=False, device=DEV)
    _check_names(c, pr_c, pr_o)
    return CC.run_program(pr_c, rings_c, c, xs, DEV), CC.run_program(pr_o, rings_o, c, xs, DEV)


@pytest.mark.parametrize("name", [c["name"] for c in CC.CASES if c["C"] in (32, 64)])
def test_chain_is_bit_identical_to_the_rows_kernel_on_real_values(gpu, name):
    """Gaussian inputs and weights of both signs through the chain program and through its per-op twin on conv_rl16: every output and every
    live history row equal, every call."""
    from audiodec_amd import native
    c = CC.CASE_BY_NAME[name]
    _assert_plan(c, native)
    ws, bs, xs = CC.real_operands(c)
    got_c, got_o = _run_pair(c, ws, bs, xs)
    for i, ((yc, hc, fc), (yo, ho, fo)) in enumerate(zip(got_c, got_o)):
        ctx = (name, "call", i)
        assert fc == 0 and fo == 0, ctx
        assert bool(torch.isfinite(yo).all()) and float(yo.abs().max()) > 0.1, ctx
        _same(yc, yo, ctx + ("output",))
        for k, (a, b) in enumerate(zip(hc, ho)):
            _same(a, b, ctx + ("history of node", k))
    assert native.device_flags() == 0


@pytest.mark.parametrize("name", ["128 one stream K7, T 32, 128 workgroups", "128 two tiles K7, two streams, B 43 odd x 3 groups, T 25",
                                  "128 two streams one tile K11 dilation 4 / 5, signed, B 129 odd, T 5 .. 15",
                                  "128 two streams one tile ELU dilation 6 / 9 (history 36 / 54), T 12"])
def test_chain_at_128_channels_on_real_values(gpu, name):
    """128 channels on Gaussian operands stays under the bound of the whole-model test (tests/test_gpu_b256.py: 2e-5 once a 128-channel chain
    has run), here relative to the largest output: the per-op kernel at this width is the stream-K kernel, which splits K across workgroups --
    another association of the same sums, so no per-op kernel sums in the chain's order -- and ELU's negative side cannot be put on a grid.
    What the chain does to real values at this width -- the activation and the split -- is rb_put8<C, ACT> / lds_put, one template for all three
    widths, which the 32- and 64-channel cases above pin bit for bit."""
    from audiodec_amd import native
    c = CC.CASE_BY_NAME[name]
    _assert_plan(c, native)
    ws, bs, xs = CC.real_operands(c)
    got_c, got_o = _run_pair(c, ws, bs, xs)
    worst = 0.0
    for (yc, hc, fc), (yo, ho, fo) in zip(got_c, got_o):
        assert fc == 0 and fo == 0
        scale = float(yo.abs().max())
        assert scale > 0.1
        for a, b in [(yc, yo)] + [(a, b) for a, b in zip(hc, ho) if a.numel()]:          # (no history in front of a 1x1 conv)
            assert a.shape == b.shape
            worst = max(worst, float((a - b).abs().max()) / scale)
    print(f"{name}: max |chain - per-op| / max |output| = {worst:.2e}")
    assert worst <= 2e-5
    assert native.device_flags() == 0


def test_calls_of_one_program_land_in_different_arms(gpu):
    """max_frames = 3 at 32 channels, 129 steps per frame: one frame runs on the `few` two-tile arm, two on the three-tile arm, three on the
    four-tile arm -- each continuing from the ring state the other arms left, exact against the model."""
    from audiodec_amd import native
    c = CC.case("mixed arms", 5, 32, "K7", 2, 129, 3, kind="signed", slope=0.5, frames=[3, 1, 2, 3, 2, 1, 1, 2, 3], seed=101)
    arms = {f: CC.plan(c, f, native=native)["arm"] for f in (1, 2, 3)}
    assert arms == {1: 2, 2: 4, 3: 5}, arms
    calls, _ = CC.run_model(c)
    ws, bs, xs = CC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr, rings = CC.build_program(c, ws, bs, chain=True, device=DEV)
    for f in (1, 2, 3):
        assert CC.chain_op_names(pr, f)[1] == "conv_rb16<32>"
    for i, (call, (y, hist, flags)) in enumerate(zip(calls, CC.run_program(pr, rings, c, xs, DEV))):
        assert flags == 0
        _same(y, call["out"][cls], ("mixed arms", i, "arm", arms[call["frames"]], "output"))
        for k, h in enumerate(hist):
            _same(h, call["hist"][k][cls], ("mixed arms", i, "arm", arms[call["frames"]], "history of node", k))


@pytest.mark.parametrize("C, rate", [(64, 257), (128, 65)])
def test_a_refused_call_runs_op_by_op_and_still_matches(gpu, C, rate):
    """T = 257 at 64 channels and T = 65 at 128 need five / three tiles per wave: the plan refuses, the chain program falls back to per-op
    launches at run time (describe_op names no conv_rb16), and the results still equal the model."""
    from audiodec_amd import native
    c = CC.case(f"refused {C}", 0, C, "K3", 2, rate, 1, kind="signed", slope=0.5, frames=[1] * 6, seed=102 + C)
    assert not CC.plan(c, native=native)["taken"]
    calls, _ = CC.run_model(c)
    ws, bs, xs = CC.operands(c)
    cls, _ = CC.stream_classes(c["B"])
    pr, rings = CC.build_program(c, ws, bs, chain=True, device=DEV)
    names = CC.chain_op_names(pr, 1)
    assert not any("rb16" in n for n in names), names
    for i, (call, (y, hist, flags)) in enumerate(zip(calls, CC.run_program(pr, rings, c, xs, DEV))):
        assert flags == 0
        _same(y, call["out"][cls], (c["name"], i, "output"))
        for k, h in enumerate(hist):
            _same(h, call["hist"][k][cls], (c["name"], i, "history of node", k))
