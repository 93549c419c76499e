"""CPU side of the residual-chain tests: the launch plan swept over every shape class, and proof that the comparison of
tests/test_gpu_chain_variants.py is sharp (tests/chain_cases.py: the case table, the exact model, the f32 emulation).

The plan query (adk_conv_rb16_plan) is host logic of the library: these tests need the built library, not a GPU."""
import functools
import itertools

import pytest
import torch

import chain_cases as CC

T_SWEEP = [1, 5, 12, 16, 17, 25, 32, 33, 64, 65, 100, 128, 129, 192, 193, 256, 257, 300, 384, 385, 512, 513]
SWEEP_DILS = {"K11": (1, 3, 5), "K7": (1, 6, 9), "K3": (1, 3, 5), "ELU": (1, 3, 9)}        # the longest histories the models use: 50, 54, 10, 54 rows


@pytest.fixture(scope="module")
def native():
    from audiodec_amd import native
    native.lib()
    return native


def _plan(native, C, tapset, dils, B, G, T):
    ta, tb, act = CC.TAPSETS[tapset]
    d = [x for u in dils for x in (u, 1)]
    return native.conv_rb16_plan(C, ta, tb, CC.ACT_ELU if act == "ELU" else CC.ACT_LEAKY, d, B, G, T)


@pytest.fixture(scope="module")
def sweep(native):
    """{(C, tap set, groups, B, T): plan} over the issue's grid."""
    out = {}
    for C, ts, G, T in itertools.product((32, 64, 128), CC.TAPSETS, (1, 3), T_SWEEP):
        for B in range(1, 401):
            out[(C, ts, G, B, T)] = _plan(native, C, ts, SWEEP_DILS[ts], B, G, T)
    return out


def test_the_plan_reaches_exactly_the_arms_the_gpu_cases_cover(sweep, native):
    """Every (arm, tap set) pair some shape of the sweep reaches has an exact-model GPU case, and every pair the case table claims is reached
    -- an instantiation nobody can reach, or one no case covers, fails here.  The arm ids are those of the header."""
    reached = {(p["arm"], ts) for (C, ts, G, B, T), p in sweep.items() if p["taken"]}
    assert {a for a, _ in reached} == set(CC.ARMS) == set(native.RB16_ARMS), sorted({a for a, _ in reached})
    assert reached == CC.COVERED, (sorted(reached - CC.COVERED), sorted(CC.COVERED - reached))
    # K11 at three tiles has an arm of its own (the residual fetched behind the second conv's loop); every other arm is built for all four tap sets
    assert {ts for a, ts in reached if a == 3} == {"K11"} and {ts for a, ts in reached if a == 4} == {"K7", "K3", "ELU"}
    assert len(reached) == 4 * 10 + 1 + 3


def test_every_plan_fits_the_history_staging_of_its_instantiation(sweep):
    """hist_issue / hist_commit of csrc/conv_rb16.hip stop at the piece count of the instantiation (SMAX streams of 56 rows): a plan that needs
    more -- two streams with more than 32 history rows in the one-stream build, as the parent's dispatch had it -- would lose history rows
    without a flag.  Recomputed here from the plan's geometry, not taken from the library's own count."""
    for (C, ts, G, B, T), p in sweep.items():
        if not p["taken"]:
            continue
        ta, tb, _ = CC.TAPSETS[ts]
        hist = max(max((ta - 1) * d, tb - 1) for d in SWEEP_DILS[ts])
        cap = (CC.ARM_SMAX[p["arm"]] * CC.MAX_HIST * (C // 8) + 255) // 256 * 256
        need = p["spw"] * hist * (C // 8)
        assert p["max_hist"] == hist and p["hist_needed"] == need and p["hist_capacity"] == cap, (C, ts, G, B, T, p)
        assert need <= cap and p["spw"] <= CC.ARM_SMAX[p["arm"]], (C, ts, G, B, T, p)
    two_in_one = [k for k, p in sweep.items() if p["taken"] and p["arm"] == 12]
    assert two_in_one and all(sweep[k]["spw"] == 2 and sweep[k]["n_tiles"] == 1 and k[4] <= 16 and k[3] * k[2] > 128 for k in two_in_one)


def test_the_plan_follows_the_documented_geometry(sweep):
    """Independent of the library's ladder: tiles per wave from T, the ring exactly where two tiles meet more than 128 workgroups (which is why
    the 168-register two-tile builds WITHOUT a ring could not be reached and were deleted), warm-up touches at 129 .. 384 workgroups of 32 / 64
    channels, helpers up to 64 workgroups, LDS within 160 KiB."""
    for (C, ts, G, B, T), p in sweep.items():
        if not p["taken"]:
            continue
        wm = 4 // (C // 32)
        assert p["workgroups"] == -(-B // p["spw"]) * G and p["n_tiles"] == -(-p["spw"] * T // 32)
        assert p["ntw"] == max(1 if C == 128 else 2, -(-p["n_tiles"] // wm)) and p["few"] == (p["workgroups"] <= 128)
        if C in (32, 64) and p["ntw"] == 2:
            assert (p["ring_slots"] == 3) == (not p["few"]) and p["arm"] == {(32, 0): 1, (32, 1): 2, (64, 0): 6, (64, 1): 7}[(C, p["few"])]
        else:
            assert p["ring_slots"] == 0
        assert p["warm"] == (C <= 64 and 128 < p["workgroups"] <= 384)
        assert (p["helpers"] > 0) == (p["workgroups"] <= 64) and (p["grid"] == p["workgroups"] or p["helpers"] > 0)
        assert 0 < p["lds_bytes"] <= 160 * 1024


def test_refusals_are_not_errors(native):
    """T too long, a history over 56 rows, LDS over 160 KiB, a tap set or a width the kernel is not built for: 'not taken', all words 0."""
    leaky, elu = CC.ACT_LEAKY, CC.ACT_ELU
    d6 = [1, 1, 3, 1, 5, 1]
    refused = [
        native.conv_rb16_plan(64, 11, 11, leaky, d6, 4, 1, 257),                 # five tiles per wave
        native.conv_rb16_plan(128, 11, 11, leaky, d6, 4, 1, 65),
        native.conv_rb16_plan(32, 11, 11, leaky, d6, 4, 1, 513),
        native.conv_rb16_plan(32, 11, 11, leaky, [1, 1, 6, 1], 4, 1, 25),         # history 60
        native.conv_rb16_plan(64, 7, 1, elu, [1, 1, 10, 1], 4, 1, 25),
        native.conv_rb16_plan(32, 5, 5, leaky, d6, 4, 1, 25),                    # no such tap set
        native.conv_rb16_plan(32, 7, 1, leaky, d6, 4, 1, 25),
        native.conv_rb16_plan(32, 11, 11, elu, d6, 4, 1, 25),
        native.conv_rb16_plan(96, 7, 7, leaky, d6, 4, 1, 25),
    ]
    for p in refused:
        assert not p["taken"] and not any(v for k, v in p.items() if k != "taken"), p
    # LDS: 128 channels, two streams of 32 steps behind 56 history rows is the largest launch there is -- 93 KiB, taken
    big = native.conv_rb16_plan(128, 7, 7, leaky, [9, 1, 9, 1], 200, 1, 32)
    assert big["taken"] and big["lds_bytes"] == 2 * (54 + 32) * 528 + 256
    lib = native.lib()
    out = (native.C.c_int32 * 16)()
    dd = (native.C.c_int32 * 6)(*d6)
    assert lib.adk_conv_rb16_plan(32, 11, 11, leaky, dd, 5, 4, 1, 25, out) != 0          # an odd number of convs
    assert lib.adk_conv_rb16_plan(32, 11, 11, leaky, dd, 6, 0, 1, 25, out) != 0
    assert lib.adk_conv_rb16_plan(32, 11, 11, leaky, None, 6, 4, 1, 25, out) != 0
    assert lib.adk_conv_rb16_plan(32, 11, 11, leaky, dd, 6, 4, 1, 25, None) != 0


def test_the_case_table_is_what_it_claims(native):
    """Each case reaches its arm at a full step; the two-level conv sits at every position of a chain; the protocol has >= 6 calls of mixed
    frame counts, a zeroed stream and a reset; the forms the lowerings use (x.repeat, external last ring) are there at every width they occur."""
    for c in CC.CASES:
        p = CC.plan(c, native=native)
        assert p["taken"] and p["arm"] == c["arm"], (c["name"], p)
        pr = CC.protocol(c)
        assert len(pr) >= 6 and sum(z for _, z, _ in pr) == 1 and sum(r for _, _, r in pr) == 1
    assert {c["two"] for c in CC.CASES if c["kind"] == "twolevel" and c["tapset"] != "ELU"} == set(range(6))
    assert {c["two"] for c in CC.CASES if c["tapset"] == "ELU"} == set(range(6))
    assert {c["slope"] for c in CC.CASES if c["kind"] == "signed"} == {0.5, 0.25}
    assert sum(len(set(c["frames"])) > 1 for c in CC.CASES) > len(CC.CASES) // 2
    assert {c["C"] for c in CC.CASES if c["rep"]} == {32, 64, 128} and all(c["groups"] == 3 for c in CC.CASES if c["rep"])
    assert {c["C"] for c in CC.CASES if c["ext_last"]} == {32, 64, 128}
    wg = {c["name"]: CC.plan(c, native=native) for c in CC.CASES}
    assert any(p["arm"] == 1 and p["warm"] for p in wg.values()) and any(p["arm"] == 1 and p["workgroups"] > 384 for p in wg.values())
    assert any(p["arm"] == 1 and p["workgroups"] > 256 for p in wg.values())                      # the tile rotation by blockIdx.x / 256
    assert {p["workgroups"] for p in wg.values() if p["arm"] == 2} >= {1, 9, 64, 65}
    assert any(p["arm"] == 11 and p["spw"] == 2 and CC.CASE_BY_NAME[n]["B"] % 2 for n, p in wg.items())
    assert any(p["arm"] == 12 and p["max_hist"] > 32 and p["hist_needed"] > 1024 for p in wg.values())


@pytest.mark.parametrize("name", list(CC.CASE_BY_NAME))
def test_a_shuffled_f32_chain_reproduces_the_model(name):
    """The model's preconditions hold for the case (run_model asserts them), and then an f32 chain that adds its products in a shuffled order
    over explicit rings equals the f64 model bit for bit: outputs and live history rows, every call."""
    c = CC.CASE_BY_NAME[name]
    calls, stats = CC.run_model(c)
    assert stats["share"] < 1.0
    ws, bs, xs = CC.operands(c)
    for call, (y, hist) in zip(calls, CC.emulate(c, ws, bs, xs)):
        assert torch.equal(y, call["out"]), (name, call["frames"])
        for k, h in enumerate(hist):
            assert torch.equal(h, call["hist"][k]), (name, call["frames"], k)


@functools.lru_cache(maxsize=None)
def _differs(name, fault, at=1):
    """Share of the elements a GPU case compares (outputs and live history rows of every call) on which the wrong chain is off the model."""
    c = CC.CASE_BY_NAME[name]
    calls, _ = CC.run_model(c)
    ws, bs, xs = CC.operands(c)
    bad = tot = 0
    for call, (y, hist) in zip(calls, CC.emulate(c, ws, bs, xs, fault=fault, at=at)):
        for got, want in [(y, call["out"])] + list(zip(hist, call["hist"])):
            bad += int((got != want).sum())
            tot += got.numel()
    return bad / tot


def _first(pred):
    return next(c["name"] for c in CC.CASES if pred(c))


TWO_TILE_128 = "128 two streams one tile K11 dilation 4 / 5 (history 40 / 50), T 15"
# wrong chain -> [(case that must tell it apart, the conv it is planted in)]
WRONG = {
    "hist_shift": [("32 few K7, 9 workgroups", 1), ("32 few K7, 9 workgroups", 2), ("64 few K11, 3 workgroups", 3)],
    "no_wrap": [("32 few K11, 1 workgroup", 0), (TWO_TILE_128, 0)],
    "res_prev": [("32 few K3, 64 workgroups", 0), ("64 few ELU, 1 workgroup, T 100", 0)],
    "keep_less": [("32 few K7, 9 workgroups", 0), ("128 one stream K11, T 25", 0)],
    "cut_1024": [(TWO_TILE_128, 0), ("128 two streams one tile K7 dilation 6 / 9 (history 36 / 54), T 16", 0),
                 ("128 two streams one tile ELU dilation 6 / 9 (history 36 / 54), T 12", 0),
                 ("128 two streams one tile K11 dilation 4 / 5, signed, B 129 odd, T 5 .. 15", 0)],
    # the two-level conv at every position, LeakyReLU and ELU cases: its lo weight fragments are multiplied by something
    "drop_wlo_ahi": [(_first(lambda c, j=j, e=e: c["kind"] == "twolevel" and c["two"] == j and (c["tapset"] == "ELU") == e), j) for j in range(6) for e in (False, True)],
    # the lo half of the activations: from the second conv on in the signed cases, behind the two-level conv in the others
    "drop_alo_whi": [("32 few K7, 9 workgroups", k) for k in (1, 2, 3)] + [("32 few K3, 64 workgroups", k) for k in (1, 2, 3, 4, 5)]
                    + [("32 ring K7, 387 workgroups (warm-up off)", k) for k in (1, 2, 3, 4, 5)],
    "swap_columns": [("128 two tiles K7, two streams, B 43 odd x 3 groups, T 25", 0), (TWO_TILE_128, 0)],
}


@pytest.mark.parametrize("fault", list(WRONG))
def test_wrong_chains_are_told_apart(fault):
    """Each wrong chain, planted in the emulation, is off the model on every case listed for it (the share of differing elements is printed):
    the history of a conv shifted by a row; history read without the ring wrap; the residual of the unit before; one row too few of an
    intermediate ring stored (shows in a later call); the second stream's history cut after 1024 pieces (the parent's two-streams-one-tile
    launch); w_lo a_hi or a_lo w_hi dropped in one conv; the columns of two streams in a shared tile swapped."""
    for name, at in WRONG[fault]:
        assert at < CC.n_convs(CC.CASE_BY_NAME[name])
        share = _differs(name, fault, at)
        print(f"{fault} in conv {at} of '{name}': {100 * share:.2f} % of the compared elements differ")
        assert share > 0, (fault, name, at)


def test_bias_before_the_join_is_told_apart_on_real_values():
    """On the grid every order of the additions is exact, so (m + bias) + c / 2048 equals the model; it is the bit-identity runs on Gaussian
    operands that see it -- the emulation in the kernels' own k order, right against wrong."""
    for name in ("32 few K7, 9 workgroups", "64 few K11, 3 workgroups"):
        c = CC.CASE_BY_NAME[name]
        ws, bs, xs = CC.real_operands(c)
        good = CC.emulate(c, ws, bs, xs, shuffle=False)
        again = CC.emulate(c, ws, bs, xs, shuffle=False)
        wrong = CC.emulate(c, ws, bs, xs, fault="bias_before_join", shuffle=False)
        assert all(torch.equal(a[0], b[0]) for a, b in zip(good, again))
        bad = sum(int((a[0] != b[0]).sum()) for a, b in zip(good, wrong))
        tot = sum(a[0].numel() for a in good)
        print(f"bias_before_join on '{name}': {100 * bad / tot:.2f} % of the outputs differ")
        assert bad > 0, name
        # ... and on the exact case it is invisible, as the argument says
        assert _differs(name, "bias_before_join") == 0.0
