"""CPU: the HiFi-GAN discriminator's backward to its input -- host side, and what tests/golden/disc_grad.npz means.

  * `differentiable` defaults to False everywhere, exists on every class that takes it, and the refusals stay; the natural side
    may never require grad; the UnivNet discriminator did not gain the flag;
  * adk_disc_conv_grad / adk_disc_prep_grad / adk_disc_loss_grad are in the header and bound, the ABI is 14, and their argument
    checks run on the host before any HIP call;
  * the backward GEMM's phase weight packing against a NumPy transposed-conv restatement;
  * the fixture's reference gradients lie within their stored E_ref of the fp64 oracle at the reference's decisions (recomputed
    here for the reduced cases with the fp64 decisions where the two agree -- see the test), and the oracle with fp64 decisions
    is plain fp64 autograd of disc_oracle's formulas.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import disc_grad_oracle as GO
import disc_oracle as DO
from audiodec_amd import discriminator as D

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def test_keyword_exists_and_defaults_to_false():
    for cls in (D.HiFiGANMultiScaleDiscriminator, D.HiFiGANMultiPeriodDiscriminator, D.Discriminator,
                D.GeneratorAdversarialLoss, D.FeatureMatchLoss, D.AdversarialEval):
        p = inspect.signature(cls.__init__).parameters
        assert "differentiable" in p and p["differentiable"].default is False, cls.__name__
    assert inspect.signature(D.from_config).parameters["differentiable"].default is False
    assert "differentiable" not in inspect.signature(D.DiscriminatorAdversarialLoss.__init__).parameters
    d = D.Discriminator(**DO.PARAMS["reduced"])
    assert d.differentiable is False and d.msd.differentiable is False and d.mpd.differentiable is False
    dd = D.Discriminator(**DO.PARAMS["reduced"], differentiable=True)
    assert dd.differentiable is True and dd.msd.differentiable is True and dd.mpd.differentiable is True
    cfg = GO.eval_config("shipped")
    assert D.from_config(cfg, d).differentiable is False
    assert D.from_config(cfg, dd, differentiable=True).differentiable is True
    assert D.GeneratorAdversarialLoss().differentiable is False and D.FeatureMatchLoss().differentiable is False


def test_refusals_stay():
    x, z = torch.zeros(1, 1, 100, requires_grad=True), torch.zeros(1, 1, 100)
    d = D.Discriminator(**DO.PARAMS["reduced"])
    for call in (lambda: d(x), lambda: d.msd(x), lambda: d.mpd(x), lambda: D.GeneratorAdversarialLoss()([[x]]),
                 lambda: D.FeatureMatchLoss()([[x, x]], [[z, z]]), lambda: D.DiscriminatorAdversarialLoss()([[x]], [[z]])):
        with pytest.raises(NotImplementedError, match="forward only"):
            call()
    dd = D.Discriminator(**DO.PARAMS["reduced"], differentiable=True)
    # the natural side is a constant: refused whatever the flag says; so is everything out of scope
    with pytest.raises(NotImplementedError, match="forward only"):
        D.FeatureMatchLoss(differentiable=True)([[z, z]], [[x, x]])
    with pytest.raises(NotImplementedError, match="forward only"):
        D.DiscriminatorAdversarialLoss()([[x]], [[z]])
    # a negative slope has no output-side mask
    bad = dict(DO.PARAMS["reduced"])
    bad["scale_discriminator_params"] = dict(bad["scale_discriminator_params"], nonlinear_activation_params={"negative_slope": -0.1})
    D.Discriminator(**bad)
    with pytest.raises(ValueError, match="negative_slope >= 0"):
        D.Discriminator(**bad, differentiable=True)
    assert dd.state_dict_keys() == d.state_dict_keys()


def test_univnet_discriminator_has_no_flag_and_refuses():
    from audiodec_amd import univnet_discriminator as U
    for cls in (U.Discriminator, U.UnivNetSpectralDiscriminator, U.UnivNetMultiResolutionSpectralDiscriminator):
        assert "differentiable" not in inspect.signature(cls.__init__).parameters
    u = U.Discriminator()
    assert u.mpd.differentiable is False and not hasattr(u, "differentiable")
    with pytest.raises(NotImplementedError, match="forward only"):
        u(torch.zeros(1, 1, 4800, requires_grad=True))


def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in ("adk_disc_conv_grad", "adk_disc_prep_grad", "adk_disc_loss_grad"):
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd = C.c_void_p(16), C.c_void_p(18)      # never dereferenced: every call below fails (or finishes) before a launch

    def conv(dy=dummy, y=dummy, w=dummy, dx=dummy, n=2, cin=8, h=100, p=3, cout=16, g=4, k=5, s=3, pad=2, act=2, slope=0.1, impl=2):
        return lib.adk_disc_conv_grad(dy, y, w, dx, n, cin, h, p, cout, g, k, s, pad, act, C.c_float(slope), impl, None)

    def prep(dy=dummy, dx=dummy, rows=2, n_in=100, op=0, a=3, b=0, c=0):
        return lib.adk_disc_prep_grad(dy, dx, rows, n_in, op, a, b, c, None)

    def loss(a=dummy, b=dummy, n=10, kind=2, coef=0.5, up=dummy, out=dummy):
        return lib.adk_disc_loss_grad(a, b, n, kind, C.c_double(coef), up, out, None)

    for kw in ({"n": -1}, {"cin": 0}, {"h": 0}, {"p": 0}, {"cout": 0}, {"g": 0}, {"k": 0}, {"s": 0}, {"pad": -1}):
        assert conv(**kw) == ADK_ERR_ARG, kw
    assert conv(g=3) == ADK_ERR_ARG and b"groups must divide" in lib.adk_last_error()
    assert conv(act=1) == ADK_ERR_ARG and conv(impl=3) == ADK_ERR_ARG
    assert conv(slope=-0.1) == ADK_ERR_ARG and b"slope >= 0" in lib.adk_last_error()
    assert conv(h=2, k=41, pad=2) == ADK_ERR_ARG and b"kernel longer" in lib.adk_last_error()
    for kw in ({"dy": None}, {"y": None}, {"w": None}, {"dx": None}):
        assert conv(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"dy": odd}, {"y": odd}, {"w": odd}, {"dx": odd}):
        assert conv(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert conv(g=1, s=70000) == ADK_ERR_ARG and b"too large" in lib.adk_last_error()
    assert conv(n=0, dy=None, y=None, w=None, dx=None) == 0                      # nothing to do: no launch
    assert prep(n_in=0) == ADK_ERR_ARG and prep(rows=-1) == ADK_ERR_ARG and prep(op=2) == ADK_ERR_ARG
    assert prep(a=100) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
    assert prep(op=1, a=4, b=0, c=2) == ADK_ERR_ARG and prep(op=1, a=4, b=2, c=3) == ADK_ERR_ARG
    for kw in ({"dy": None}, {"dx": None}):
        assert prep(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"dy": odd}, {"dx": odd}):
        assert prep(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert prep(rows=0, dy=None, dx=None) == 0
    assert loss(n=-1) == ADK_ERR_ARG and loss(kind=6) == ADK_ERR_ARG and loss(kind=-1) == ADK_ERR_ARG
    for kw in ({"a": None}, {"b": None}, {"up": None}, {"out": None}):
        assert loss(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"a": odd}, {"b": odd}, {"up": odd}, {"out": odd}):
        assert loss(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert loss(n=0, a=None, b=None, up=None, out=None) == 0


def _transposed_conv_by_packing(packed, dy, L, h_in):
    """dx (C_in, H) of one item with P = 1 from the PACKED weights alone, the way the kernel walks them (numpy, float64)."""
    g, s, k, pad = L.groups, L.stride, L.kernel, L.pad
    cout_g, cin_g = L.cout // g, L.cin // g
    h_out = dy.shape[1]
    dx = np.zeros((L.cin, h_in))
    flat = packed.reshape(g, cout_g * k, cin_g)
    for gi in range(g):
        off = 0
        for r in range(s):
            nt = len(range(r, k, s))
            block = flat[gi, off:off + cout_g * nt]                                 # [kk = co * nt + tt][m]
            off += cout_g * nt
            for h in range(h_in):
                if (h + pad) % s != r:
                    continue
                u = (h + pad) // s
                for co in range(cout_g):
                    for tt in range(nt):
                        ho = u - tt
                        if 0 <= ho < h_out:
                            dx[gi * cin_g:(gi + 1) * cin_g, h] += block[co * nt + tt] * dy[gi * cout_g + co, ho]
        assert off == cout_g * k
    return dx


@pytest.mark.parametrize("cin,cout,k,s,pad,g,h", [(6, 4, 5, 3, 2, 2, 17), (4, 6, 41, 4, 20, 1, 50), (3, 2, 2, 3, 1, 1, 11),
                                                  (4, 4, 5, 1, 2, 4, 9), (2, 3, 7, 7, 3, 1, 30)])
def test_phase_weight_packing(cin, cout, k, s, pad, g, h):
    L = D.Layer("x", cin, cout, k, s, pad, g, True, None, "none", False)
    rng = np.random.default_rng(k * 100 + s)
    w = torch.from_numpy(rng.integers(-4, 5, size=L.weight_shape).astype(np.float32))
    packed = D.pack_grad_weights(w, L)
    assert tuple(packed.shape) == (g, (cout // g) * k, cin // g) and packed.is_contiguous()
    h_out = D.conv_out_len(h, L)
    dy = rng.integers(-3, 4, size=(cout, h_out)).astype(np.float64)
    x = torch.zeros(1, cin, h, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv1d(x, w.double(), None, stride=s, padding=pad, groups=g)
    y.backward(torch.from_numpy(dy)[None])
    assert np.array_equal(_transposed_conv_by_packing(packed.numpy().astype(np.float64), dy, L, h), x.grad[0].numpy())


def test_fixture_contents(fixture):
    for case, (pname, shape) in GO.CASES.items():
        for flags in GO.FLAGS:
            ref = fixture[f"{case}_{flags}_grad"]
            assert ref.shape == tuple(shape) and ref.dtype == np.float32
            eref, gmax = float(fixture[f"{case}_{flags}_eref"]), float(fixture[f"{case}_{flags}_gmax"])
            assert 0 < eref <= 1e-5 * gmax, f"{case} {flags}: E_ref {eref:.3g} against max|grad64| {gmax:.3g}"
        assert (f"{case}_bounds" in fixture.files) == (f"{case}_flips" in fixture.files) == (pname == "reduced")
    assert GO.REDUCED_CASES == ["t1203", "t11", "stereo", "b2"]


@pytest.mark.parametrize("case", ["t1203", "t11", "stereo"])
def test_bounds_are_the_forward_tests(fixture, golden_dir, case):
    """The per-layer bounds stored for the decision checks are test_gpu_discriminator._bound of the forward fixture."""
    fwd = np.load(os.path.join(golden_dir, "disc.npz"), allow_pickle=False)
    y_hat, y = GO.inputs(case)
    exact = DO.forward64("reduced", DO.state_dict("reduced"), np.concatenate([y_hat, y], 0))
    ref = [[fwd[f"{case}_d{d}_l{l}"] for l in range(len(o))] for d, o in enumerate(exact)]
    assert np.allclose(fixture[f"{case}_bounds"], GO.layer_bounds(ref, exact), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", GO.REDUCED_CASES)
def test_reference_gradient_within_eref_of_oracle(fixture, golden_dir, case):
    """Self-consistency: the stored float32 gradient lies within the stored E_ref of grad64 at the reference's decisions.  Those
    are rebuilt from the reference's float32 feature maps where the forward fixture stores them (disc.npz: three cases); the
    B = 2 case has none stored, but the fixture records that the reference took every decision there as fp64 does."""
    pname, sd = "reduced", DO.state_dict("reduced")
    y_hat, y = GO.inputs(case)
    n = y_hat.shape[0] * y_hat.shape[1]
    if case == "b2":
        assert int(fixture["b2_flips"]) == 0
        masks = signs = None                                                       # the fp64 decisions
    else:
        fwd = np.load(os.path.join(golden_dir, "disc.npz"), allow_pickle=False)
        n_l = [len(ls) for ls in D.Discriminator(**DO.PARAMS[pname]).discriminator_layers]
        ref = [[fwd[f"{case}_d{d}_l{l}"] for l in range(k)] for d, k in enumerate(n_l)]
        masks, signs = GO.decisions([[t[:n] for t in o] for o in ref], [[t[n:] for t in o] for o in ref])
    for flags in GO.FLAGS:
        g = GO.grad64(pname, sd, y_hat, y, flags, masks, signs)
        ref_g = fixture[f"{case}_{flags}_grad"].astype(np.float64)
        err, eref = float(np.max(np.abs(ref_g - g))), float(fixture[f"{case}_{flags}_eref"])
        print(f"{case} {flags}: max|ref - grad64| {err:.3g}  stored E_ref {eref:.3g}")
        assert g.shape == ref_g.shape
        assert err <= eref * (1 + 1e-9) + 1e-18
        assert float(np.max(np.abs(g))) == pytest.approx(float(fixture[f"{case}_{flags}_gmax"]), rel=1e-12)


@pytest.mark.parametrize("case", ["t11", "stereo"])
def test_oracle_with_fp64_decisions_is_plain_autograd(case):
    pname, sd = "reduced", DO.state_dict("reduced")
    y_hat, y = GO.inputs(case)
    for flags in GO.FLAGS:
        a, b = GO.grad64(pname, sd, y_hat, y, flags), GO.plain_grad64(pname, sd, y_hat, y, flags)
        assert a.shape == y_hat.shape and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    # negated signs negate the feature-matching part and leave the adversarial part alone
    with torch.no_grad():
        fh = GO.features64(pname, sd, torch.from_numpy(y_hat).double())
        fr = GO.features64(pname, sd, torch.from_numpy(y).double())
    masks, signs = GO.decisions(fh, fr)
    full = GO.grad64(pname, sd, y_hat, y, "shipped", masks, signs)
    neg = GO.grad64(pname, sd, y_hat, y, "shipped", masks, [[-s for s in o] for o in signs])
    adv = GO.grad64(pname, sd, y_hat, y, "mse_nofm", masks, signs)
    assert np.allclose(full + neg, 2 * adv, rtol=1e-9, atol=1e-15)
