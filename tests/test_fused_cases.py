"""CPU side of the fused-tail tests: proof that the comparison of tests/test_gpu_fused_exact.py is sharp (tests/fused_cases.py: the case
table, the exact model of both pairs, the f32 emulation) and that the case table reaches the edges it claims.  No GPU, no library."""
import functools

import numpy as np
import pytest
import torch

import chain_cases as CC
import fused_cases as FC

ALL = list(FC.CASE_BY_NAME) + [n + " + tanh" for n in FC.TANH_OF]


def _case(name):
    return FC.tanh_case(name[:-len(" + tanh")]) if name.endswith(" + tanh") else FC.CASE_BY_NAME[name]


@pytest.mark.parametrize("name", ALL)
def test_a_shuffled_f32_launch_reproduces_the_model(name):
    """The model's preconditions hold (run_model asserts them: splits, caps, grids, non-zero shares, live lo halves), and an f32 emulation
    of the launch that adds its products in a shuffled order over explicit rings equals the model bit for bit, every call."""
    c = _case(name)
    calls, stats = FC.run_model(c)
    assert stats["share"] < 1.0
    print(f"{name}: largest S {100 * stats['share']:.1f} % of its cap; lo live: x {stats['lo_x']:.2f} act(c) {stats['lo_a']:.2f} W1 {stats['lo_w1']:.3f} W2 {stats['lo_w2']:.3f}")
    ops, xs = FC.operands(c)
    for call, (y, hist) in zip(calls, FC.emulate(c, ops, xs)):
        assert torch.equal(y, call["out"]), (name, call["frames"])
        assert torch.equal(hist, call["hist"]), (name, call["frames"])


@functools.lru_cache(maxsize=None)
def _differs(name, fault):
    """Share of the elements a GPU case compares (outputs and live history rows of every call) on which the wrong launch is off the model."""
    c = FC.CASE_BY_NAME[name]
    calls, _ = FC.run_model(c)
    ops, xs = FC.operands(c)
    bad = tot = 0
    for call, (y, hist) in zip(calls, FC.emulate(c, ops, xs, fault=fault)):
        for got, want in ((y, call["out"]), (hist, call["hist"])):
            bad += int((got != want).sum())
            tot += got.numel()
    return bad / tot


OU_SIGNED = "ou MT2 3 (3, 32) ladder LeakyReLU 0.5 signed"
OU_NOACT = "ou MT2 2 (2, 32) ladder no activation signed, no bias 1"
OU_W1TWO = "ou MT2 1 (2, 16) ladder ELU two-level W1, no bias 2"
OU_STRADDLE = "ou (3, 32) out ring 1 + 300 rows: phases straddle the wrap"
OC_A, OC_B = "oc ladder A LeakyReLU 0.5 signed", "oc ladder B LeakyReLU 0.5 signed"
# wrong launch -> the cases that must tell it apart
WRONG = {
    "halo_late": [OU_SIGNED, OU_NOACT, OU_W1TWO],
    "halo_skip": [OU_SIGNED, OU_W1TWO],
    "hist_raw": [OU_SIGNED, "ou MT2 1 (2, 16) LeakyReLU 0.25 signed"],
    "hist_early": [OU_SIGNED, OU_NOACT, OU_W1TWO],
    "clast15": [OU_SIGNED, OU_NOACT],
    "bias2_tile": [OU_SIGNED, OU_NOACT],
    "phase_cout_g": [OU_STRADDLE, "ou (8, 4) out ring 2 + 264 rows, two-level x"],
    "swizzle": [OU_SIGNED, OU_NOACT, OU_W1TWO],
    "drop_alo_whi2": [OU_SIGNED, OU_W1TWO, "ou MT2 2 (2, 32) LeakyReLU two-level x, no biases"],
    "act_lo_dropped": [OU_SIGNED, OU_W1TWO],
    "store_past_T": [OU_STRADDLE],
    "lead_from_ring": [OC_A, OC_B],
    "slice0_recomputed": [OC_A, OC_B],
    "to_ring_short": [OC_A, OC_B],
    "hist_activated": [OC_A, OC_B],
    "taps_reversed": [OC_A, OC_B, "oc ladder A ELU two-level W1, no output bias"],
    "last_slice_len": [OC_A, OC_B],
    "bias1_on_hist": [OC_A, OC_B],
    "drop_xlo_whi": [OC_A, "oc ladder B LeakyReLU two-level x"],
    "drop_xhi_wlo": ["oc ladder A ELU two-level W1, no output bias"],
}


def test_every_listed_fault_has_cases():
    assert set(WRONG) == set(FC.OU_FAULTS) | set(FC.OC_FAULTS)


@pytest.mark.parametrize("fault", list(WRONG))
def test_wrong_launches_are_told_apart(fault):
    """Each wrong kernel, planted in the emulation (fused_cases._emulate_ou / _emulate_oc say what each one is), is off the model on every
    case listed for it; the share of differing elements is printed."""
    for name in WRONG[fault]:
        assert FC.CASE_BY_NAME[name]["pair"] == ("ou" if fault in FC.OU_FAULTS else "oc")
        share = _differs(name, fault)
        print(f"{fault} on '{name}': {100 * share:.3f} % of the compared elements differ")
        assert share > 0, (fault, name)


def test_the_float_phase_formula_is_integer_division_for_every_admitted_pair():
    """(int)((ml + 0.5f) * (1.0f / cout_real)) of conv_ou16 / conv_up16 in float32 equals ml // cout_real for all 14 (up, cout_real)."""
    assert len(FC.ADMITTED) == 14 and {(3, 32), (24, 4), (2, 48), (16, 4)} <= set(FC.ADMITTED)
    for up, co in FC.ADMITTED:
        ml = np.arange(up * co, dtype=np.float32)
        inv = np.float32(1.0) / np.float32(co)
        ph = ((ml + np.float32(0.5)) * inv).astype(np.float32).astype(np.int32)
        assert np.array_equal(ph, np.arange(up * co) // co), (up, co)


def test_the_case_table_is_what_it_claims():
    """Every MT2 with at least two (up, cout_real) pairs, the pairs the phase formula is extreme at, both T ladders in full, every
    activation arm and bias combination per MT2, the stream counts, a straddling output ring, a protocol with a zeroed stream and a reset."""
    ou = [c for c in FC.CASES if c["pair"] == "ou"]
    oc = [c for c in FC.CASES if c["pair"] == "oc"]
    for c in FC.CASES:
        pr = CC.protocol(c)
        assert len(pr) >= 6 and sum(z for _, z, _ in pr) == 1 and sum(r for _, _, r in pr) == 1
        assert len(set(c["frames"])) > 1 or c["B"] >= 257
        assert (c["up"], c["cout"]) in FC.ADMITTED or c["pair"] == "oc"
        assert all(1 <= f * c["rate"] <= (FC.OU_TMAX if c["pair"] == "ou" else 366) for f in c["frames"])
        assert c["B"] <= 5 or c["B"] >= 257
    pairs = {(c["up"], c["cout"]) for c in ou}
    assert pairs >= {(2, 16), (8, 4), (4, 16), (2, 32), (3, 32), (8, 12), (24, 4)}
    for mt2 in (1, 2, 3):
        mine = [c for c in ou if c["up"] * c["cout"] == 32 * mt2]
        assert len({(c["up"], c["cout"]) for c in mine}) >= 2
        assert {c["act"] for c in mine} == {None, "LeakyReLU", "ELU"}
        assert {(c["b1"], c["b2"]) for c in mine} == {(True, True), (False, True), (True, False), (False, False)}
        for act in (None, "LeakyReLU", "ELU"):
            steps = {f * c["rate"] for c in mine if c["act"] == act for f in c["frames"]}
            assert steps >= {1, 2, 15, 16, 17, 100, 127, 128}, (mt2, act)
        assert any(c["kind"] == "signed" and c["act"] == "LeakyReLU" for c in mine)
    assert {c["kind"] for c in ou} == {"signed", "w1two", "xtwo", "w2two"} and {c["slope"] for c in ou if c["kind"] == "signed" and c["act"]} == {0.5, 0.25}
    assert any(c["out_hist"] and (c["out_hist"] + c["F"] * c["rate"] * c["up"]) % c["up"] for c in ou)
    assert {1, 3} <= {c["B"] for c in ou} and any(c["B"] >= 257 for c in ou)
    steps = {f * c["rate"] for c in oc for f in c["frames"]}
    assert steps >= {1, 2, 5, 6, 7, 26, 27, 121, 122, 123, 244, 245, 300, 366}
    assert {c["act"] for c in oc} == {None, "LeakyReLU", "ELU"} and {c["kind"] for c in oc} == {"signed", "w1two", "xtwo"}
    assert any(not c["b1"] and c["b2"] for c in oc) and any(c["b1"] and not c["b2"] for c in oc)
    assert {1, 3} <= {c["B"] for c in oc} and any(c["B"] * FC.slices(c["F"] * c["rate"])[0] > 768 for c in oc)
    assert FC.slices(122) == (1, 122) and FC.slices(123) == (2, 62) and FC.slices(244) == (2, 122) and FC.slices(245) == (3, 82) and FC.slices(366) == (3, 122)
    for frames in (FC.OC_LADDER_A, FC.OC_LADDER_B):           # a T = 1 call between longer ones: the six-step history comes from several calls
        assert any(frames[i] == 1 and frames[i - 1] < 6 and frames[i + 1] > 1 for i in range(1, len(frames) - 1))
    assert all(FC.CASE_BY_NAME[n]["pair"] == "oc" and FC.CASE_BY_NAME[n]["act_out"] is None for n in FC.TANH_OF)


@pytest.mark.parametrize("name", list(FC.UNIT_BY_NAME))
def test_the_residual_unit_cases_hold_their_preconditions(name):
    """The one-unit chain_cases programs behind the fused residual unit: the model's preconditions hold and the shuffled f32 emulation of
    tests/chain_cases.py reproduces it."""
    c = FC.UNIT_BY_NAME[name]
    calls, stats = CC.run_model(c)
    assert stats["share"] < 1.0 and CC.n_convs(c) == 2 and (c["ta"], c["tb"]) == (7, 1)
    ws, bs, xs = CC.operands(c)
    for call, (y, hist) in zip(calls, CC.emulate(c, ws, bs, xs)):
        assert torch.equal(y, call["out"]), (name, call["frames"])
        assert all(torch.equal(h, w) for h, w in zip(hist, call["hist"])), (name, call["frames"])


def test_the_residual_unit_cases_reach_every_launch_form():
    """One, two, three and four items on four waves, five on five waves, more than five and fewer than 24 steps declined."""
    items = {FC.unit_items(c["C"], c["dils"][0], c["B"], f * c["rate"]) for c in FC.UNIT_CASES for f in c["frames"]}
    assert items == {None, 1, 2, 3, 4, 5, 6}, items
    assert {c["C"] for c in FC.UNIT_CASES if FC.unit_items(c["C"], c["dils"][0], c["B"], c["F"] * c["rate"]) == 6} == {32, 64}
    assert {c["kind"] for c in FC.UNIT_CASES} == {"signed", "twolevel"}
