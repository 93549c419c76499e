"""GPU: the HiFi-GAN discriminator's backward to its input (adk_disc_conv_grad, adk_disc_prep_grad, adk_disc_loss_grad).

  A. op level, exact: small integer-valued weights, inputs and upstream gradients make every f32 sum exact, so each op must
     torch.equal the f64 autograd of its torch restatement cast to f32 -- over the shapes that can break the indexing;
  B. decisions: LeakyReLU masks and L1 signs taken from the HIP forward's feature maps differ from the fp64 ones only at elements
     whose fp64 margin is within the forward test's bound for that layer;
  C. gradient: for every case and flag set of disc_grad_oracle, max|hip - grad64(HIP's decisions)| <= 4 E_ref + 1e-6 max|grad64|,
     E_ref the reference's own float32 error at its own decisions (disc_grad.npz);
  D. bitwise reproducibility; AdversarialEval(differentiable=True) against the forward-only call and against the separate classes;
     graph construction; the second backward.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_grad_oracle as GO
import disc_oracle as DO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def forward_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc.npz"), allow_pickle=False)


# ---- A. op level ----
# (n_items, c_in, c_out, kernel, stride, pad, groups, h_in, period, leaky, forced impl)
CONV_CASES = {
    "s1_k5_cin3_n128_k25": (2, 3, 5, 5, 1, 2, 1, 64, 1, True, None),           # C_out/g * taps = 25: no multiple of 16
    "s1_cin32_n127": (1, 32, 6, 5, 1, 2, 1, 127, 1, True, None),               # one full M tile
    "s1_cin33_n129": (1, 33, 4, 5, 1, 2, 1, 129, 1, True, None),               # M tile edge, second N tile of one column
    "s1_n1": (1, 4, 4, 5, 1, 2, 1, 1, 1, True, None),                          # a single input position
    "s1_items_in_tile": (3, 4, 4, 5, 1, 2, 1, 50, 1, True, None),              # item boundaries at columns 50 and 100 of tile 0
    "s3_k5_p3_tail": (2, 4, 8, 5, 3, 2, 1, 20, 3, True, None),                 # H + 2 pad - k = 19: the last row is never read
    "s3_k5_p3_tail_direct": (2, 4, 8, 5, 3, 2, 1, 20, 3, True, "direct"),
    "s4_k41_g4_tail": (2, 8, 16, 41, 4, 20, 4, 103, 1, True, None),            # span 102: two rows never read
    "s4_k41_g4_p1_short": (1, 8, 8, 41, 4, 20, 4, 3, 1, True, None),           # fewer rows than phases
    "k2_s3_empty_phase": (1, 4, 6, 2, 3, 1, 1, 20, 1, True, None),             # kernel < stride: phase 2 has no taps
    "s3_cin64_tile": (2, 64, 8, 5, 3, 2, 1, 200, 2, True, None),               # the 64 x 128 tile, several column blocks
    "s1_cin128_tile_noact": (1, 128, 4, 3, 1, 1, 1, 40, 1, False, None),       # the 128 x 128 tile, no activation
    "first_layer_cin1": (2, 1, 8, 15, 1, 7, 1, 100, 1, True, None),            # direct: dx is the waveform gradient
    "first_layer_cin1_split": (1, 1, 64, 5, 3, 2, 1, 31, 3, True, None),       # direct, C_out/g split over 8 threads
    "depthwise_s2": (1, 4, 8, 5, 2, 2, 4, 33, 1, True, None),                  # direct, C_in/g = 1 with groups
    "output_cout1": (2, 16, 1, 3, 1, 1, 1, 50, 1, False, None),                # direct: the scale output conv
    "output_cout1_k2_p3": (2, 8, 1, 2, 1, 1, 1, 10, 3, False, None),           # direct: the period output conv, H + 1 rows
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_grad_exact(gpu, name):
    from audiodec_amd import discriminator as D
    n, cin, cout, k, s, pad, g, h, p, leaky, forced = CONV_CASES[name]
    L = D.Layer("op", cin, cout, k, s, pad, g, True, 0.5 if leaky else None, "none", p != 1)
    rng = np.random.default_rng(sum(CONV_CASES[name][:9]))
    w = torch.from_numpy(rng.integers(-3, 4, size=L.weight_shape).astype(np.float32))
    b = torch.from_numpy(rng.integers(-2, 3, size=cout).astype(np.float32))
    x = torch.from_numpy(rng.integers(-4, 5, size=(n, cin, h, p)).astype(np.float32))
    ho = D.conv_out_len(h, L)
    dy = torch.from_numpy(rng.integers(-3, 4, size=(n, cout, ho, p)).astype(np.float32))
    conv = D._Conv(L, w, b, gpu)
    if forced == "direct":
        assert conv.impl == D.IMPL_GEMM
        conv.impl, conv.w = D.IMPL_DIRECT, w.contiguous().to(gpu)
    else:
        assert conv.impl == (D.IMPL_DIRECT if cin // g == 1 or cout // g == 1 else D.IMPL_GEMM)
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(xr, w.double()[..., None], b.double(), stride=(s, 1), padding=(pad, 0), groups=g)
    if leaky:
        yr = F.leaky_relu(yr, 0.5)
    yr.backward(dy.double())
    xg = x.to(gpu).requires_grad_(True)
    y = D._ConvFn.apply(xg, conv)
    assert y.requires_grad and torch.equal(y.detach().cpu(), yr.detach().float())
    y.backward(dy.to(gpu))
    assert xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
    assert torch.equal(xg.grad.cpu(), xr.grad.float()), f"{name}: max diff {float((xg.grad.cpu() - xr.grad.float()).abs().max())}"
    assert float(xr.grad.abs().max()) > 0


@pytest.mark.parametrize("rows,n_in,n_pad", [(3, 11, 10), (2, 12, 1), (1, 1203, 7), (2, 2, 1), (1, 300, 299)])
def test_reflect_grad_exact(gpu, rows, n_in, n_pad):
    from audiodec_amd import discriminator as D
    rng = np.random.default_rng(n_in)
    x = torch.from_numpy(rng.integers(-4, 5, size=(rows, n_in)).astype(np.float32))
    dy = torch.from_numpy(rng.integers(-3, 4, size=(rows, n_in + n_pad)).astype(np.float32))
    xr = x.double().requires_grad_(True)
    F.pad(xr[None], (0, n_pad), "reflect")[0].backward(dy.double())
    xg = x.to(gpu).requires_grad_(True)
    y = D._prep_op(xg, rows, n_in, D.PREP_REFLECT, n_pad, n_out=n_in + n_pad, grad=True)
    assert torch.equal(y.detach().cpu(), F.pad(x[None], (0, n_pad), "reflect")[0])
    y.backward(dy.to(gpu))
    assert torch.equal(xg.grad.cpu(), xr.grad.float())


@pytest.mark.parametrize("rows,n_in,k,s,p", [(3, 11, 4, 2, 2), (2, 1203, 4, 2, 2), (1, 2, 4, 2, 2), (2, 30, 2, 2, 0), (2, 33, 4, 4, 1),
                                             (1, 50, 8, 3, 4), (2, 9, 4, 1, 2)])
def test_avgpool_grad_exact(gpu, rows, n_in, k, s, p):
    from audiodec_amd import discriminator as D
    rng = np.random.default_rng(n_in + k)
    n_out = D.pool_out_len(n_in, k, s, p)
    x = torch.from_numpy(rng.integers(-4, 5, size=(rows, n_in)).astype(np.float32))
    dy = torch.from_numpy(rng.integers(-3, 4, size=(rows, n_out)).astype(np.float32))
    xr = x.double().requires_grad_(True)
    F.avg_pool1d(xr[None], k, s, p)[0].backward(dy.double())
    xg = x.to(gpu).requires_grad_(True)
    y = D._prep_op(xg, rows, n_in, D.PREP_AVGPOOL, k, s, p, n_out=n_out, grad=True)
    assert torch.equal(y.detach().cpu(), F.avg_pool1d(x[None], k, s, p)[0])
    y.backward(dy.to(gpu))
    assert torch.equal(xg.grad.cpu(), xr.grad.float())


@pytest.mark.parametrize("kind", range(6))
def test_loss_grad_exact(gpu, kind):
    """c = coef * upstream = -0.125 exactly; the values include every decision point (1, -1, v == b)."""
    from audiodec_amd import discriminator as D
    from audiodec_amd import native
    rng = np.random.default_rng(kind)
    a = np.concatenate([np.array([1.0, -1.0, 0.0, 1.5, -1.5, 0.75, -0.75], np.float32),
                        (rng.integers(-8, 9, size=1030) / 4).astype(np.float32)])
    b = np.concatenate([np.array([1.0, -1.0, 0.0, 0.5, -2.0, 0.75, 0.25], np.float32),
                        (rng.integers(-8, 9, size=1030) / 4).astype(np.float32)])
    assert (a == b).sum() > 10 and (a != b).sum() > 500
    want = [2 * (a - 1), 2 * a, np.sign(a - b), np.ones_like(a), (a < 1).astype(np.float32), -(a > -1).astype(np.float32)][kind]
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    up = torch.tensor([-0.5], device=gpu)
    out = torch.full_like(ta, 7.0)
    native.check(native.lib().adk_disc_loss_grad(D._ptr(ta), D._ptr(tb) if kind == D.LOSS_L1 else None, ta.numel(), kind, 0.25,
                                                 D._ptr(up), D._ptr(out), native.current_stream(ta.device)), "adk_disc_loss_grad")
    assert torch.equal(out.cpu(), torch.from_numpy((-0.125 * want).astype(np.float32)))
    if kind < 4:                                                   # and torch's own derivative of the term (sign(0) = 0)
        x = torch.from_numpy(a).double().requires_grad_(True)
        y = torch.from_numpy(b).double()
        [(x - 1) ** 2, x ** 2, (x - y).abs(), x][kind].sum().mul(-0.125).backward()
        assert torch.equal(out.cpu(), x.grad.float())


# ---- B, C: the whole network ----
_DISCS, _STATE = {}, {}


def _disc(pname, gpu, differentiable=True):
    from audiodec_amd import discriminator as D
    key = (pname, differentiable)
    if key not in _DISCS:
        _DISCS[key] = D.Discriminator(**DO.PARAMS[pname], device=gpu, differentiable=differentiable).load_state_dict(DO.state_dict(pname))
    return _DISCS[key]


def _eval(pname, flags, gpu, differentiable=True):
    from audiodec_amd import discriminator as D
    return D.from_config(GO.eval_config(flags), _disc(pname, gpu, differentiable), differentiable=differentiable)


def _state(case, gpu):
    """Per case, once: the inputs, the HIP forward's feature maps' decisions, and the fp64 feature maps' decisions and margins."""
    if case not in _STATE:
        pname = GO.CASES[case][0]
        y_hat, y = GO.inputs(case)
        sd = DO.state_dict(pname)
        with torch.no_grad():
            d = _disc(pname, gpu)
            hip_hat = [[t.cpu().numpy() for t in o] for o in d(torch.from_numpy(y_hat).to(gpu))]
            hip = [[t.cpu().numpy() for t in o] for o in d(torch.from_numpy(y).to(gpu))]
            f64_hat = [[GO._np(t) for t in o] for o in GO.features64(pname, sd, torch.from_numpy(y_hat).double())]
            f64 = [[GO._np(t) for t in o] for o in GO.features64(pname, sd, torch.from_numpy(y).double())]
        _STATE[case] = dict(pname=pname, sd=sd, y_hat=y_hat, y=y, hip=GO.decisions(hip_hat, hip), f64=GO.decisions(f64_hat, f64),
                            margins=GO.margins64(f64_hat, f64), f64_cat=[[np.concatenate([a, b], 0) for a, b in zip(oh, o)]
                                                                         for oh, o in zip(f64_hat, f64)])
    return _STATE[case]


def _hip_grad(case, flags, gpu):
    st = _state(case, gpu)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    v = _eval(st["pname"], flags, gpu)(a, torch.from_numpy(st["y"]).to(gpu))
    (GO.UPSTREAM * v["adversarial_loss"]).backward()
    return v, a.grad


@pytest.mark.parametrize("case", list(GO.CASES))
def test_decisions_differ_from_fp64_only_within_the_forward_bound(gpu, fixture, forward_fixture, case):
    st = _state(case, gpu)
    if case in GO.REDUCED_CASES:
        bounds = fixture[f"{case}_bounds"]
    else:                                            # from the stored samples, as the forward test does
        bounds = []
        for d, o in enumerate(st["f64_cat"]):
            for l, t in enumerate(o):
                ex = t.reshape(-1)[DO.sample_index(t.size)]
                ref = forward_fixture[f"{case}_d{d}_l{l}_sample"]
                bounds.append(4 * np.max(np.abs(ref - ex)) + 1e-6 * max(1.0, float(np.max(np.abs(ex)))))
    found, ok = GO.disagreements(*st["hip"], *st["f64"], st["margins"], bounds)
    for d, l, what, n, worst, bound in found:
        print(f"{case} d{d} l{l}: {n} {what} decisions differ from fp64, worst fp64 margin {worst:.3g}, bound {bound:.3g}")
    print(f"{case}: {sum(f[3] for f in found)} decisions differ from fp64")
    assert ok, f"{case}: a HIP decision differs from fp64 at an element outside the forward bound: {found}"


@pytest.mark.parametrize("flags", list(GO.FLAGS))
@pytest.mark.parametrize("case", list(GO.CASES))
def test_gradient_against_fp64_at_hip_decisions(gpu, fixture, case, flags):
    st = _state(case, gpu)
    v, grad = _hip_grad(case, flags, gpu)
    assert grad.shape == st["y_hat"].shape and grad.dtype == torch.float32 and v["adversarial_loss"].requires_grad
    exact = GO.grad64(st["pname"], st["sd"], st["y_hat"], st["y"], flags, *st["hip"])
    eref, gmax = float(fixture[f"{case}_{flags}_eref"]), float(fixture[f"{case}_{flags}_gmax"])
    err, bound = float(np.max(np.abs(grad.cpu().numpy().astype(np.float64) - exact))), 4 * eref + 1e-6 * gmax
    print(f"{case} {flags}: max|hip - grad64| {err:.3g}  E_ref {eref:.3g}  max|grad64| {gmax:.3g}  ratio to bound {err / bound:.3f}")
    assert err <= bound, f"{case} {flags}: max|hip - grad64| {err:.3g} > {bound:.3g}"


# ---- D ----
def test_bitwise_reproducible(gpu):
    for flags in ("shipped", "hinge_avg"):
        (v1, g1), (v2, g2) = _hip_grad("t1203", flags, gpu), _hip_grad("t1203", flags, gpu)
        assert torch.equal(g1, g2) and all(torch.equal(v1[k], v2[k]) for k in v1)
        assert float(g1.abs().max()) > 0 and torch.isfinite(g1).all()


@pytest.mark.parametrize("case", ["t1203", "stereo", "b2"])
def test_adversarial_eval_values_are_the_forward_only_ones(gpu, case):
    st = _state(case, gpu)
    a, b = torch.from_numpy(st["y_hat"]).to(gpu), torch.from_numpy(st["y"]).to(gpu)
    for flags in GO.FLAGS:
        with torch.no_grad():
            plain = _eval(st["pname"], flags, gpu, differentiable=False)(a, b)
            quiet = _eval(st["pname"], flags, gpu)(a.clone().requires_grad_(True), b)      # no_grad: the forward-only pass
        v = _eval(st["pname"], flags, gpu)(a.clone().requires_grad_(True), b)
        assert list(v) == list(plain) and set(v) == set(quiet)
        print(f"{case} {flags}: bitwise equal to the forward-only call: {all(torch.equal(v[k].detach(), plain[k]) for k in v)}")
        for k in v:
            assert v[k].dim() == 0 and v[k].dtype == torch.float32
            assert float(v[k].detach()) == pytest.approx(float(plain[k]), rel=1e-6), f"{flags} {k}"
            assert torch.equal(quiet[k], plain[k]) and not quiet[k].requires_grad
            assert v[k].requires_grad == (k in ("adversarial_loss", "feature_matching_loss")), k
        # an input that does not require grad: the plain forward
        w = _eval(st["pname"], flags, gpu)(a, b)
        assert all(torch.equal(w[k], plain[k]) and not w[k].requires_grad for k in w)


@pytest.mark.parametrize("flags", list(GO.FLAGS))
def test_adversarial_eval_gradient_is_the_separate_classes(gpu, fixture, flags):
    from audiodec_amd import discriminator as D
    st = _state("b2", gpu)
    _, g_eval = _hip_grad("b2", flags, gpu)
    f = GO.FLAGS[flags]
    d = _disc("reduced", gpu)
    a, b = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True), torch.from_numpy(st["y"]).to(gpu)
    with torch.no_grad():
        p = d(b)
    p_ = d(a)
    assert all(t.grad_fn is not None for o in p_ for t in o) and all(not t.requires_grad for o in p for t in o)
    loss = D.GeneratorAdversarialLoss(*f["gen"], differentiable=True)(p_)
    if f["fm"] is not None:
        loss = loss + f["lambda_feat_match"] * D.FeatureMatchLoss(*f["fm"], differentiable=True)(p_, p)
    assert loss.requires_grad and loss.dtype == torch.float32
    (GO.UPSTREAM * f["lambda_adv"] * loss).backward()
    gmax = float(fixture[f"b2_{flags}_gmax"])
    # the same kernels on the same decisions; the scalar factors are rounded in a different order (a few f32 roundings per term)
    assert float((a.grad - g_eval).abs().max()) <= 1e-6 * gmax
    # the natural side's feature maps may not require grad, and a forward-only loss refuses the graph
    with pytest.raises(NotImplementedError, match="forward only"):
        D.GeneratorAdversarialLoss(*f["gen"])(d(a))


def test_graph_only_when_asked(gpu):
    st = _state("t11", gpu)
    d, plain = _disc("reduced", gpu), _disc("reduced", gpu, differentiable=False)
    a = torch.from_numpy(st["y_hat"]).to(gpu)
    outs = d(a)                                                                    # does not require grad: no graph
    assert all(t.grad_fn is None and not t.requires_grad for o in outs for t in o)
    with torch.no_grad():
        quiet = d(a.clone().requires_grad_(True))
        ref = plain(a)
    graph = d(a.clone().requires_grad_(True))
    for o, q, r, gph in zip(outs, quiet, ref, graph):
        for t, u, v, w in zip(o, q, r, gph):
            assert torch.equal(t, v) and torch.equal(u, v) and torch.equal(w.detach(), v)
            assert not u.requires_grad and w.grad_fn is not None
    with pytest.raises(NotImplementedError, match="forward only"):
        plain(a.clone().requires_grad_(True))
    # a feature map's own gradient and the gradient of what follows it are added by autograd
    x = a.clone().requires_grad_(True)
    o = d.msd(x)[0]
    (o[2].sum() + o[-1].sum()).backward()
    g_both = x.grad.clone()
    x.grad = None
    o = d.msd(x)[0]
    o[2].sum().backward()
    g_mid = x.grad.clone()
    x.grad = None
    d.msd(x)[0][-1].sum().backward()
    assert float((g_both - (g_mid + x.grad)).abs().max()) <= 1e-5 * float(g_both.abs().max())


def test_double_backward(gpu):
    st = _state("t11", gpu)
    b = torch.from_numpy(st["y"]).to(gpu)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    v = _eval("reduced", "shipped", gpu)(a, b)["adversarial_loss"]
    (g,) = torch.autograd.grad(v, a, create_graph=True)
    assert not g.requires_grad                                   # the gradient is a constant to autograd
    with pytest.raises(RuntimeError, match="does not require grad"):
        g.sum().backward()
    # an upstream gradient that itself requires grad asks for the second derivative: once_differentiable's error
    w = torch.ones((), device=gpu, requires_grad=True)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    (g,) = torch.autograd.grad(_eval("reduced", "shipped", gpu)(a, b)["adversarial_loss"] * w, a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
