"""GPU: the HiFi-GAN discriminator's own update (adk_disc_conv_wgrad, discriminator_train.TrainableDiscriminator and its
DiscriminatorAdversarialLoss).

  A. exact: small-integer x, dy, y (exact zeros included) and slope 0.5 / 0.25 make every f32 sum exact, so dW and db must
     torch.equal the f64 restatement -- over the channel shapes, (kernel, stride, pad), periods, reduction lengths and flag
     combinations that can break the indexing, on outputs and a workspace full of NaN; a split reduction; n_items == 0;
  B. group isolation: NaN in one group's x, dy or both leaves the other groups' dW and db bitwise what they were;
  C. real values, slope 0.1, against f64 within 4 E + 1e-6 max, E the error of torch's own f32 CPU run of the same op;
  D. the differentiable DiscriminatorAdversarialLoss: values bitwise the forward-only class's, gradients within 1e-6 max of f64;
  E. whole discriminator: every parameter's gradient of every case and flag set of disc_train.npz within 4 E_ref + 1e-6 gmax of
     the f64 oracle at the HIP forward's decisions; the feature maps bitwise discriminator.Discriminator's;
  F. reproducibility, accumulation, launch counts of the discriminator step and of the generator step, one Adam step.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_oracle as DO
import disc_train_oracle as TO

pytestmark = pytest.mark.gpu
NONE, LEAKY = 0, 2


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_train.npz"), allow_pickle=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nan(gpu, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _h_out(h_in, k, s, pad):
    return (h_in + 2 * pad - k) // s + 1


def _wgrad(gpu, dy, y, x, G, k, s, pad, act, slope, want_db=True):
    """adk_disc_conv_wgrad on outputs and a workspace full of NaN -> (dw, db, slices)."""
    from audiodec_amd import discriminator_train as T
    from audiodec_amd import native
    n, cin, h_in, period = x.shape
    cout = dy.shape[1]
    nb, slices = T.conv_wgrad_plan(n, cin, h_in, period, cout, G, k, s, pad)
    ws = _nan(gpu, max(1, nb // 4))
    dw, db = _nan(gpu, cout, cin // G, k), (_nan(gpu, cout) if want_db else None)
    dyg, yg, xg = (a.to(gpu).contiguous() if a is not None and a.numel() else None for a in (dy, y, x))
    native.check(native.lib().adk_disc_conv_wgrad(_p(dyg), _p(yg if act == LEAKY else None), _p(xg), _p(dw), _p(db), _p(ws), n, cin,
                                                  h_in, period, cout, G, k, s, pad, act, C.c_float(slope),
                                                  native.current_stream(gpu)), "adk_disc_conv_wgrad")
    return dw, db, slices


def _ref(dy, y, x, G, k, s, pad, act, slope, dt):
    """(dW, db) by torch autograd of F.conv2d in dtype dt on the CPU, the mask taken as y > 0 ? 1 : slope (slope the float32
    the kernel is given, whatever dt is)."""
    cout, cin_g = dy.shape[1], x.shape[1] // G
    dz = dy.to(dt) * (torch.where(y > 0, 1.0, slope).to(dt) if act == LEAKY else 1.0)
    w = torch.zeros(cout, cin_g, k, 1, dtype=dt, requires_grad=True)
    if x.shape[0]:
        F.conv2d(x.to(dt), w, None, stride=(s, 1), padding=(pad, 0), groups=G).backward(dz)
        dw = w.grad[..., 0]
    else:
        dw = torch.zeros(cout, cin_g, k, dtype=dt)
    return dw, dz.sum((0, 2, 3))


# ---- A. exact ----
CH = [(1, 1, 32), (1, 33, 1), (3, 5, 5), (4, 33, 33), (1, 64, 32), (1, 8, 64), (2, 4, 130)]        # (groups, c_in/g, c_out/g)
KSP = [(15, 1, 7), (41, 4, 20), (5, 3, 2), (3, 1, 1), (2, 1, 1), (3, 4, 1)]                        # (kernel, stride, pad)
PERIODS, ITEMS = [1, 2, 3, 11], [1, 3]
FLAGSETS = [(NONE, False), (NONE, True), (LEAKY, False), (LEAKY, True)]                            # (act, db given)
TARGETS = ["h1", "h2", "r31", "r32", "r33", "tail"]


def _exact_cases():
    """One case per (channel shape, (kernel, stride, pad)); the period, n_items, the flags and what h_in aims at rotate so that
    every value meets every tile shape (32 rows: c_out/g < 64, 64 rows: (1, 8, 64), 128 rows: (2, 4, 130))."""
    out = {}
    for c, (G, cig, cog) in enumerate(CH):
        for i, (k, s, pad) in enumerate(KSP):
            target = TARGETS[(i + c) % 6]
            period, n = PERIODS[(i + c) % 4], ITEMS[(i + c // 2) % 2]
            act, want_db = FLAGSETS[(i + 2 * c) % 4]
            ho = {"h1": 1, "h2": 2, "r31": 31, "r32": 16, "r33": 1, "tail": 3}[target]
            if target == "r31":
                period, n = 1, 1
            elif target == "r32":
                period, n = 2, 1
            elif target == "r33":
                period, n = 11, 3
            h_in = max(1, (ho - 1) * s + k - 2 * pad) + (s - 1 if target in ("h2", "tail") else 0)     # + s - 1: rows the forward never reads
            slope = 0.5 if (i + c) % 2 else 0.25
            out[f"g{G}_{cig}x{cog}_k{k}s{s}p{pad}_P{period}_n{n}_h{h_in}_{target}_a{act}{'b' if want_db else ''}"] = \
                (G, cig, cog, k, s, pad, period, h_in, n, act, want_db, slope)
    return out


EXACT = _exact_cases()


def _tile(cog):
    return 128 if cog >= 128 else 64 if cog >= 64 else 32


def test_exact_cases_cover_the_list():
    for tile in (32, 64, 128):
        cs = [v for v in EXACT.values() if _tile(v[2]) == tile]
        assert {v[3:6] for v in cs} == set(KSP) and {v[6] for v in cs} == set(PERIODS) and {v[8] for v in cs} == set(ITEMS), tile
        assert {(v[9], v[10]) for v in cs} == set(FLAGSETS), tile
        ho = {_h_out(v[7], *v[3:6]) for v in cs}
        red = {v[8] * _h_out(v[7], *v[3:6]) * v[6] for v in cs}
        assert {1, 2} <= ho and {31, 32, 33} <= red, (tile, ho, red)
        assert any((v[7] + 2 * v[5] - v[3]) % v[4] for v in cs), tile
    assert {v[:3] for v in EXACT.values()} == set(CH)


def _int_operands(seed, G, cig, cog, k, s, pad, period, h_in, n):
    rng = np.random.default_rng(seed)
    ho = _h_out(h_in, k, s, pad)
    ints = lambda lo, hi, shape: torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))      # noqa: E731
    dy, y, x = ints(-3, 3, (n, G * cog, ho, period)), ints(-2, 2, (n, G * cog, ho, period)), ints(-3, 3, (n, G * cig, h_in, period))
    y.view(-1)[::3] = 0.0                                  # exact zeros: the mask's y == 0 side
    return dy, y, x


@pytest.mark.parametrize("name", list(EXACT))
def test_wgrad_exact(gpu, name):
    G, cig, cog, k, s, pad, period, h_in, n, act, want_db, slope = EXACT[name]
    dy, y, x = _int_operands(list(name.encode()), G, cig, cog, k, s, pad, period, h_in, n)
    assert bool((y == 0).any())
    dw, db, _ = _wgrad(gpu, dy, y, x, G, k, s, pad, act, slope, want_db)
    rw, rb = _ref(dy, y, x, G, k, s, pad, act, slope, torch.float64)
    assert torch.equal(dw.cpu(), rw.float()), name
    assert db is None or torch.equal(db.cpu(), rb.float()), name


@pytest.mark.parametrize("tile", [32, 64, 128])
def test_wgrad_exact_split_reduction(gpu, tile):
    """S >= 3 slices from the plan, the last one ending inside a 32-deep step."""
    G, cig, cog = {32: (2, 3, 7), 64: (1, 8, 64), 128: (1, 4, 130)}[tile]
    k, s, pad, period, n, h_in = 5, 3, 2, 3, 3, 127       # h_out = 43: a reduction of 3 * 43 * 3 = 387 = 12 * 32 + 3 terms
    dy, y, x = _int_operands(tile, G, cig, cog, k, s, pad, period, h_in, n)
    dw, db, slices = _wgrad(gpu, dy, y, x, G, k, s, pad, LEAKY, 0.5)
    red = n * _h_out(h_in, k, s, pad) * period
    assert slices >= 3 and red % 32 != 0 and red > 12 * 32, (slices, red)
    rw, rb = _ref(dy, y, x, G, k, s, pad, LEAKY, 0.5, torch.float64)
    assert torch.equal(dw.cpu(), rw.float()) and torch.equal(db.cpu(), rb.float())


@pytest.mark.parametrize("want_db", [False, True])
def test_wgrad_no_items(gpu, want_db):
    x, dy = torch.zeros(0, 6, 9, 2), torch.zeros(0, 9, 3, 2)
    dw, db, _ = _wgrad(gpu, dy, dy, x, 3, 5, 3, 2, LEAKY, 0.1, want_db)
    assert dw.shape == (9, 2, 5) and not dw.any() and (db is None or (db.shape == (9,) and not db.any()))


# ---- B. group isolation ----
@pytest.mark.parametrize("where", ["x", "dy", "both"])
def test_wgrad_group_isolation(gpu, where):
    G, cig, cog, k, s, pad, period, h_in, n = 3, 5, 5, 5, 3, 2, 3, 20, 2
    rng = np.random.default_rng(7)
    ho = _h_out(h_in, k, s, pad)
    dy, y, x = (torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
                for sh in ((n, G * cog, ho, period), (n, G * cog, ho, period), (n, G * cig, h_in, period)))
    base_w, base_b, _ = _wgrad(gpu, dy, y, x, G, k, s, pad, LEAKY, 0.1)
    x2, dy2 = x.clone(), dy.clone()
    if where in ("x", "both"):
        x2[:, cig:2 * cig] = float("nan")
    if where in ("dy", "both"):
        dy2[:, cog:2 * cog] = float("nan")
    dw, db, _ = _wgrad(gpu, dy2, y, x2, G, k, s, pad, LEAKY, 0.1)
    others = [r for r in range(G * cog) if not cog <= r < 2 * cog]
    assert torch.equal(dw[others], base_w[others]) and torch.equal(db[others], base_b[others])
    assert bool(torch.isnan(dw[cog:2 * cog]).all())
    if where == "x":
        assert torch.equal(db[cog:2 * cog], base_b[cog:2 * cog])          # db does not read x
    else:
        assert bool(torch.isnan(db[cog:2 * cog]).all())


# ---- C. real values ----
# (groups, c_in/g, c_out/g, kernel, stride, pad, period, h_in, n_items, act)
REAL = {
    "tile128_period": (1, 32, 128, 5, 3, 2, 3, 100, 2, LEAKY),
    "tile64_grouped_k41": (4, 8, 64, 41, 4, 20, 1, 300, 2, LEAKY),
    "tile32": (1, 32, 32, 5, 3, 2, 2, 150, 2, LEAKY),
    "first_layer_scale": (1, 1, 16, 15, 1, 7, 1, 600, 2, LEAKY),
    "first_layer_period": (1, 1, 32, 5, 3, 2, 11, 60, 2, LEAKY),
    "output_conv_scale": (1, 64, 1, 3, 1, 1, 1, 80, 2, NONE),
    "output_conv_period": (1, 64, 1, 2, 1, 1, 5, 9, 2, NONE),
}


@pytest.mark.parametrize("name", list(REAL))
def test_wgrad_real_values(gpu, name):
    G, cig, cog, k, s, pad, period, h_in, n, act = REAL[name]
    rng = np.random.default_rng(list(name.encode()))
    ho = _h_out(h_in, k, s, pad)
    dy, y, x = (torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
                for sh in ((n, G * cog, ho, period), (n, G * cog, ho, period), (n, G * cig, h_in, period)))
    dw, db, _ = _wgrad(gpu, dy, y, x, G, k, s, pad, act, 0.1)
    w64, b64 = _ref(dy, y, x, G, k, s, pad, act, 0.1, torch.float64)
    w32, b32 = _ref(dy, y, x, G, k, s, pad, act, 0.1, torch.float32)
    for what, got, f32, f64 in (("dW", dw, w32, w64), ("db", db, b32, b64)):
        e_ref = float((f32.double() - f64).abs().max())
        err, bound = float((got.cpu().double() - f64).abs().max()), 4 * e_ref + 1e-6 * float(f64.abs().max())
        print(f"{name} {what}: max|hip - f64| {err:.3g}  E {e_ref:.3g}  max {float(f64.abs().max()):.3g}  fraction of the bound {err / bound:.3f}")
        assert err <= bound, f"{name} {what}: {err:.3g} > {bound:.3g}"


# ---- D. the loss ----
def _finals(gpu, seed):
    """Final outputs of three sub-discriminators straddling -1 and 1, none within 1e-3 of either."""
    rng = np.random.default_rng(seed)
    outs = []
    for shape in ((2, 37), (2, 1, 19), (2, 300)):
        v = rng.standard_normal(shape) * 1.5
        for edge in (-1.0, 1.0):
            near = np.abs(v - edge) < 1e-3
            v[near] = edge + 2e-3
        assert ((v > 1) .any() and (v < -1).any() and (np.abs(v) < 1).any())
        outs.append(torch.from_numpy(v.astype(np.float32)).to(gpu))
    return outs


@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("loss_type", ["mse", "hinge"])
def test_discriminator_loss_values_and_gradients(gpu, loss_type, avg):
    from audiodec_amd import discriminator as D
    from audiodec_amd import discriminator_train as T
    hats, reals = _finals(gpu, 1), _finals(gpu, 2)
    with torch.no_grad():
        want = D.DiscriminatorAdversarialLoss(avg, loss_type)([[t] for t in hats], [[t] for t in reals])
    lh, lr = [t.clone().requires_grad_(True) for t in hats], [t.clone().requires_grad_(True) for t in reals]
    crit = T.DiscriminatorAdversarialLoss(avg, loss_type)
    real, fake = crit([[t] for t in lh], [[t] for t in lr])
    assert torch.equal(real, want[0]) and torch.equal(fake, want[1]) and real.requires_grad and fake.requires_grad
    (0.37 * real + 1.25 * fake).backward()
    h64, r64 = [t.detach().cpu().double().requires_grad_(True) for t in hats], [t.detach().cpu().double().requires_grad_(True) for t in reals]
    if loss_type == "mse":
        r = sum(torch.mean((t - 1) ** 2) for t in r64)
        f = sum(torch.mean(t ** 2) for t in h64)
    else:
        r = sum(-torch.mean(torch.min(t - 1, torch.zeros_like(t))) for t in r64)
        f = sum(-torch.mean(torch.min(-t - 1, torch.zeros_like(t))) for t in h64)
    if avg:
        r, f = r / 3, f / 3
    (0.37 * r + 1.25 * f).backward()
    for got, ref in zip(lh + lr, h64 + r64):
        err, gmax = float((got.grad.cpu().double() - ref.grad).abs().max()), float(ref.grad.abs().max())
        assert gmax > 0 and err <= 1e-6 * gmax, (loss_type, avg, err, gmax)
    with torch.no_grad():                                  # nothing asks for a gradient: the forward-only values, no graph
        r0, f0 = crit([[t] for t in hats], [[t] for t in reals])
    assert torch.equal(r0, want[0]) and torch.equal(f0, want[1]) and not r0.requires_grad


# ---- E. whole discriminator ----
_MODELS, _RUNS = {}, {}


def _model(pname, gpu):
    from audiodec_amd import discriminator_train as T
    if pname not in _MODELS:
        m = T.TrainableDiscriminator(**DO.PARAMS[pname], device=gpu)
        m.load_state_dict(DO.state_dict(pname))
        _MODELS[pname] = m
    return _MODELS[pname]


def _step(case, flags, gpu):
    """One discriminator step's backward on the HIP path: (feature maps of y_hat, of y, {key: gradient})."""
    from audiodec_amd import discriminator_train as T
    pname = TO.CASES[case][0]
    m = _model(pname, gpu)
    y_hat, y = TO.inputs(case)
    m.zero_grad(set_to_none=True)
    p_, p = m(torch.from_numpy(y_hat).to(gpu)), m(torch.from_numpy(y).to(gpu))
    real, fake = T.DiscriminatorAdversarialLoss(**TO.loss_params(flags))(p_, p)
    (TO.UPSTREAM * (real + fake)).backward()
    return p_, p, {k: q.grad.clone() for k, q in m.named_parameters()}


def _exact(case, p_, p):
    """grads64 of the shipped flag set at the HIP forward's decisions, once per case (the averaged flag set's loss is that
    one divided by the number of sub-discriminators, and so is its gradient)."""
    if case not in _RUNS:
        pname = TO.CASES[case][0]
        y_hat, y = TO.inputs(case)
        _RUNS[case] = TO.grads64(pname, DO.state_dict(pname), y_hat, y, "shipped", TO.masks_of(p_), TO.masks_of(p))
    return _RUNS[case]


@pytest.mark.parametrize("flags", list(TO.FLAGS))
@pytest.mark.parametrize("case", list(TO.CASES))
def test_parameter_gradients_against_fp64_at_hip_decisions(gpu, fixture, case, flags):
    pname = TO.CASES[case][0]
    p_, p, grads = _step(case, flags, gpu)
    exact = _exact(case, p_, p)
    scale = 1.0 / len(p) if TO.FLAGS[flags][1] else 1.0
    names = [str(k) for k in fixture[f"{pname}_names"]]
    assert sorted(names) == sorted(grads)
    eref, gmax = fixture[f"{case}_{flags}_eref"], fixture[f"{case}_{flags}_gmax"]
    worst = (0.0, None)
    for i, k in enumerate(names):
        got, want = grads[k].cpu().numpy().astype(np.float64).reshape(-1), exact[k].reshape(-1) * scale
        if pname != "reduced":
            idx = TO.param_index(want.size, False)
            got, want = got[idx], want[idx]
        err, bound = float(np.max(np.abs(got - want))), 4 * float(eref[i]) + 1e-6 * float(gmax[i])
        worst = max(worst, (err / bound, k))
        assert err <= bound, f"{case} {flags} {k}: max|hip - grad64| {err:.3g} > {bound:.3g}"
    print(f"{case} {flags}: largest fraction of the bound {worst[0]:.3f} ({worst[1]})")


@pytest.mark.parametrize("case", ["t1203", "stereo", "v1"])
def test_forward_is_the_eval_discriminators(gpu, case):
    from audiodec_amd import discriminator as D
    pname = TO.CASES[case][0]
    m = _model(pname, gpu)
    ref = D.Discriminator(**DO.PARAMS[pname], device=gpu).load_state_dict(m.state_dict())
    x = torch.from_numpy(TO.inputs(case)[0]).to(gpu)
    with torch.no_grad():
        want, got = ref(x), m(x)
    with_graph = m(x)
    assert len(got) == len(want) == len(with_graph) == 8
    for o_w, o_g, o_t in zip(want, got, with_graph):
        assert len(o_w) == len(o_g) == len(o_t)
        for a, b, c in zip(o_w, o_g, o_t):
            assert not b.requires_grad and c.requires_grad
            assert torch.equal(a, b) and torch.equal(a, c.detach())


# ---- F. behaviour ----
class _Counter:
    """Counts the calls of one native entry point through a wrapper on the loaded library object."""

    def __init__(self, name):
        from audiodec_amd import native
        self.lib, self.name, self.calls = native.lib(), name, 0
        self.orig = getattr(self.lib, name)

    def __enter__(self):
        def wrapped(*a):
            self.calls += 1
            return self.orig(*a)
        setattr(self.lib, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)


def _counted(fn):
    with _Counter("adk_disc_conv_wgrad") as a, _Counter("adk_disc_conv_grad") as b, _Counter("adk_disc_prep_grad") as c:
        fn()
    return a.calls, b.calls, c.calls


def test_reproducible_and_accumulates(gpu):
    _, _, g1 = _step("t1203", "shipped", gpu)
    p_, p, g2 = _step("t1203", "shipped", gpu)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    from audiodec_amd import discriminator_train as T
    m = _model("reduced", gpu)
    y_hat, y = TO.inputs("t1203")
    real, fake = T.DiscriminatorAdversarialLoss(**TO.loss_params("shipped"))(m(torch.from_numpy(y_hat).to(gpu)), m(torch.from_numpy(y).to(gpu)))
    (TO.UPSTREAM * (real + fake)).backward()               # a second backward of a new graph adds to .grad
    assert all(torch.equal(q.grad, g1[k] + g1[k]) for k, q in m.named_parameters())       # g + g is exact
    m.zero_grad(set_to_none=True)


def test_launch_counts_of_both_steps(gpu):
    from audiodec_amd import discriminator as D
    from audiodec_amd import discriminator_train as T
    m = _model("reduced", gpu)
    y_hat, y = (torch.from_numpy(a).to(gpu) for a in TO.inputs("t1203"))
    n_layers = sum(len(ls) for ls in m.discriminator_layers)
    n_sub = len(m.discriminator_layers)
    crit = T.DiscriminatorAdversarialLoss(**TO.loss_params("shipped"))
    # the discriminator step: two passes, a weight gradient per layer and pass, dx for every layer but each sub-discriminator's first
    m.zero_grad(set_to_none=True)
    real, fake = crit(m(y_hat), m(y))
    assert _counted(lambda: (real + fake).backward()) == (2 * n_layers, 2 * (n_layers - n_sub), 0)
    # the generator step: frozen parameters, the waveform asks: no weight gradient, dx down to the waveform
    m.zero_grad(set_to_none=True)
    for q in m.parameters():
        q.requires_grad_(False)
    try:
        with torch.no_grad():
            assert not m(y_hat)[0][-1].requires_grad
        assert not m(y_hat)[0][-1].requires_grad              # nothing asks for a gradient: no graph
        ref = D.Discriminator(**DO.PARAMS["reduced"], device=gpu, differentiable=True).load_state_dict(m.state_dict())
        gen = D.GeneratorAdversarialLoss(average_by_discriminators=False, differentiable=True)
        a, b = y_hat.clone().requires_grad_(True), y_hat.clone().requires_grad_(True)
        loss = gen(m(a))
        # t1203: 1203 is a multiple of 3 only: four of the five periods reflect-pad, and two of the three scales are pooled
        assert _counted(lambda: loss.backward()) == (0, n_layers, 4 + 2)
        gen(ref(b)).backward()
        assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0
        assert all(q.grad is None for q in m.parameters())
    finally:
        for q in m.parameters():
            q.requires_grad_(True)


def test_adam_step_and_round_trip(gpu):
    from audiodec_amd import discriminator as D
    from audiodec_amd import discriminator_train as T
    m = T.TrainableDiscriminator(**DO.PARAMS["reduced"], device=gpu)
    m.load_state_dict(DO.state_dict("reduced"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    y_hat, y = (torch.from_numpy(a).to(gpu) for a in TO.inputs("b2"))
    opt = torch.optim.Adam(m.parameters(), lr=2.0e-4, betas=(0.5, 0.9))
    crit = T.DiscriminatorAdversarialLoss(**TO.loss_params("shipped"))
    with torch.no_grad():
        first = m(y)
    real, fake = crit(m(y_hat), m(y))
    opt.zero_grad()
    (real + fake).backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
    opt.step()
    after = m.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in before)
    ref = D.Discriminator(**DO.PARAMS["reduced"], device=gpu).load_state_dict(after)
    with torch.no_grad():
        want, got = ref(y), m(y)
    assert all(torch.equal(a, b) for o_w, o_g in zip(want, got) for a, b in zip(o_w, o_g))
    assert any(not torch.equal(a, b) for o_f, o_g in zip(first, got) for a, b in zip(o_f, o_g))      # the packings followed the step
