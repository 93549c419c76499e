"""CPU: the trainable HiFi-GAN discriminator (audiodec_amd/discriminator_train.py, csrc/disc_wgrad.hip) without a device:
  * adk_disc_conv_wgrad and its plan are in the header, exported and bound, the ABI version is unchanged, and every argument
    check runs before any HIP call;
  * the plan restated in Python, and equal to adk_voc_conv_wgrad_plan's where the two layers coincide;
  * a NumPy walk of the kernel's index mapping (the dy / y element, the x element with its validity test, the workspace row of a
    (group, row, column, rho), the slices) against torch f64 autograd of F.conv2d with the leaky mask;
  * construction: the reference's parameter names and shapes, the round trip into discriminator.Discriminator, spectral norm;
  * the weight-norm composition's g / v gradients against torch.nn.utils.weight_norm in f64 on a 4-D weight;
  * the fixture's caps, from the stored numbers.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_oracle as DO
import disc_train_oracle as TO
from audiodec_amd import discriminator as D
from audiodec_amd import discriminator_train as T

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("adk_disc_conv_wgrad_plan", "adk_disc_conv_wgrad")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_train.npz"), allow_pickle=False)


# ---- the C ABI ----
def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    # the calls are additions: the ABI version every other suite pins is unchanged
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd = C.c_void_p(16), C.c_void_p(18)           # never dereferenced: every call fails before a launch
    base = dict(n=2, cin=8, h=50, p=3, cout=16, g=2, k=5, s=3, pad=2)

    def plan(**kw):
        a = dict(base, **kw)
        ws, sl = C.c_int64(0), C.c_int32(0)
        return lib.adk_disc_conv_wgrad_plan(a["n"], a["cin"], a["h"], a["p"], a["cout"], a["g"], a["k"], a["s"], a["pad"],
                                            C.byref(ws), C.byref(sl))

    def wgrad(**kw):
        a = dict(base, dy=dummy, y=dummy, x=dummy, dw=dummy, db=dummy, ws=dummy, act=2, slope=0.1)
        a.update(kw)
        return lib.adk_disc_conv_wgrad(a["dy"], a["y"], a["x"], a["dw"], a["db"], a["ws"], a["n"], a["cin"], a["h"], a["p"], a["cout"],
                                       a["g"], a["k"], a["s"], a["pad"], a["act"], C.c_float(a["slope"]), None)

    assert plan() == 0
    for name, fn in (("adk_disc_conv_wgrad_plan", plan), ("adk_disc_conv_wgrad", wgrad)):
        for kw in (dict(n=-1), dict(cin=0), dict(h=0), dict(p=0), dict(cout=0), dict(g=0), dict(k=0), dict(s=0), dict(pad=-1)):
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        assert fn(g=3) == ADK_ERR_ARG and b"groups must divide" in lib.adk_last_error(), name
        assert fn(h=2, k=7, pad=2) == ADK_ERR_ARG and b"kernel longer than the padded input" in lib.adk_last_error(), name
        for kw in (dict(h=1 << 30), dict(pad=1 << 29, k=1), dict(n=1 << 12, h=1 << 20, p=1, s=1), dict(h=1 << 22, p=1 << 9),
                   dict(cin=1 << 16, cout=1 << 16, g=1, k=1 << 14, h=1 << 14, pad=0, p=1),          # c_in * kernel
                   dict(cin=1 << 12, cout=1 << 12, g=1, k=129, h=129, pad=0, p=1, s=1),            # c_out (ck + 1) = 2^12 (2^12 * 129 + 1)
                   dict(cin=1 << 10, g=1, h=1 << 21, p=1),                                          # the x offsets: c_in * h_in * P = 2^31
                   dict(g=1, cin=1, cout=1 << 22, k=1, pad=0, h=1, p=1, s=1, n=1)):                # the grid's y
            assert fn(**kw) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), (name, kw)
        # 2^17 groups of one tile each: one slice per group is already more than the grid's z holds
        assert fn(g=1 << 17, cin=1 << 17, cout=1 << 17, k=1, pad=0, h=1, p=1, s=1, n=1) == ADK_ERR_ARG
        assert b"groups * slices" in lib.adk_last_error(), name
    for kw in (dict(act=1), dict(act=3), dict(act=-1)):
        assert wgrad(**kw) == ADK_ERR_ARG and b"act must be 0 (none) or 2 (leaky)" in lib.adk_last_error(), kw
    assert wgrad(slope=-0.1) == ADK_ERR_ARG and b"slope >= 0" in lib.adk_last_error()
    assert wgrad(slope=float("nan")) == ADK_ERR_ARG and b"slope >= 0" in lib.adk_last_error()
    for p in ("dy", "y", "x", "dw", "ws"):
        assert wgrad(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), p
    for p in ("dy", "y", "x", "dw", "db", "ws"):
        assert wgrad(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), p
    # n_items == 0 reads nothing, but still writes: dw and the workspace are required
    assert wgrad(n=0, dy=None, y=None, x=None, dw=None) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error()
    assert wgrad(n=0, dy=None, y=None, x=None, ws=None) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error()


# ---- the plan ----
def _plan_py(n, cin, h, p, cout, g, k, s, pad):
    """The header's rule: (workspace bytes, slices)."""
    ho = (h + 2 * pad - k) // s + 1
    m, ck = cout // g, (cin // g) * k
    bm = 128 if m >= 128 else 64 if m >= 64 else 32
    tiles = g * -(-m // bm) * -(-(ck + 1) // 128)
    steps = -(-(n * ho * p) // 32)
    s0 = max(1, min(-(-512 // tiles), steps // 4))
    per = max(1, -(-steps // s0))
    slices = max(1, -(-steps // per))
    return 4 * slices * cout * (ck + 1), slices, per


PLAN_SHAPES = [(2, 8, 50, 3, 16, 2, 5, 3, 2), (32, 1, 9600, 1, 128, 1, 15, 1, 7), (32, 128, 2400, 1, 512, 16, 41, 4, 20),
               (32, 1024, 13, 3, 1024, 1, 5, 1, 2), (32, 1024, 13, 11, 1, 1, 2, 1, 1), (3, 4, 127, 3, 130, 1, 5, 3, 2),
               (0, 8, 50, 3, 16, 2, 5, 3, 2), (1, 4, 1, 1, 4, 1, 1, 1, 0), (1, 64, 33, 1, 64, 1, 3, 4, 1)]


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_plan_restated(lib, shape):
    assert T.conv_wgrad_plan(*shape) == _plan_py(*shape)[:2]


@pytest.mark.parametrize("n,cin,cout,g,k,t_out", [(2, 8, 16, 2, 5, 333), (32, 128, 128, 4, 41, 600), (1, 64, 1, 1, 3, 31), (3, 1, 32, 1, 15, 11)])
def test_plan_is_the_vocoders_where_the_layers_coincide(lib, n, cin, cout, g, k, t_out):
    """period 1, stride 1, pad 0: h_out = h_in - kernel + 1; the causal conv's t_out = t.  The same reduction length, the same plan."""
    from audiodec_amd import vocoder_train as VT
    assert T.conv_wgrad_plan(n, cin, t_out + k - 1, 1, cout, g, k, 1, 0) == VT.conv_wgrad_plan(n, cin, t_out, cout, k, 1, g)


# ---- the index mapping ----
def _walk(dy, y, x, G, k, s, pad, slope, want_db):
    """disc_wgrad_kernel's addressing on flat arrays, element by element: returns (dW, db) from the workspace rows the kernel
    writes, folded in slice order."""
    n, cout, ho, p = dy.shape
    _, cin, h_in, _ = x.shape
    cin_g, cout_g = cin // G, cout // G
    hp_in, hp_out, ck = h_in * p, ho * p, cin_g * k
    red = n * hp_out
    _, slices, per = _plan_py(n, cin, h_in, p, cout, G, k, s, pad)
    nc_live = ck + 1 if want_db else ck
    fdy, fy, fx = dy.reshape(-1), y.reshape(-1), x.reshape(-1)
    ws = np.full((slices, cout, ck + 1), np.nan)
    for grp in range(G):
        row_g, ch_g = grp * cout_g, grp * cin_g
        for sl in range(slices):
            acc = np.zeros((cout_g, nc_live))
            for rho in range(sl * per * 32, min(red, (sl + 1) * per * 32)):
                item, rem = divmod(rho, hp_out)
                h2, j = divmod(rem, p)
                ybase = item * cout * hp_out + rem
                a = np.empty(cout_g)
                for m in range(cout_g):
                    off = ybase + (row_g + m) * hp_out
                    a[m] = fdy[off] * (1.0 if slope is None or fy[off] > 0 else slope)
                b = np.zeros(nc_live)
                hb, q = h2 * s, h2 * s * p + j
                for col in range(nc_live):
                    if col == ck:
                        b[col] = 1.0
                        continue
                    ci, t = divmod(col, k)
                    xoff = (ch_g + ci) * hp_in + (t - pad) * p
                    if 0 <= hb + t - pad < h_in:
                        b[col] = fx[item * cin * hp_in + xoff + q]
                acc += np.outer(a, b)
            ws[sl, row_g:row_g + cout_g, :nc_live] = acc
    total = ws[:, :, :nc_live].sum(0)
    assert not np.isnan(total).any()                       # every live element of every slice was written
    return total[:, :ck].reshape(cout, cin_g, k), (total[:, ck] if want_db else None)


@pytest.mark.parametrize("shape", [(2, 2, 3, 2, 5, 3, 2, 3, 20, True, True), (1, 1, 1, 4, 41, 4, 20, 1, 70, True, False),
                                   (3, 1, 4, 1, 2, 1, 1, 11, 4, False, True), (2, 3, 2, 2, 3, 4, 1, 2, 30, True, True),
                                   (1, 1, 2, 3, 15, 1, 7, 1, 200, True, True)])
def test_index_mapping_against_autograd(shape):
    n, G, cin_g, cout_g, k, s, pad, p, h_in, leaky, want_db = shape
    rng = np.random.default_rng(list(shape))
    ho = (h_in + 2 * pad - k) // s + 1
    dy, y = rng.standard_normal((n, G * cout_g, ho, p)), rng.standard_normal((n, G * cout_g, ho, p))
    x = rng.standard_normal((n, G * cin_g, h_in, p))
    y.reshape(-1)[::4] = 0.0
    slope = 0.1 if leaky else None
    dw, db = _walk(dy, y, x, G, k, s, pad, slope, want_db)
    w = torch.zeros(G * cout_g, cin_g, k, dtype=torch.float64, requires_grad=True)
    dz = torch.from_numpy(dy * np.where(y > 0, 1.0, 0.1) if leaky else dy)        # the mask at y == 0 is the slope
    F.conv2d(torch.from_numpy(x), w[..., None], stride=(s, 1), padding=(pad, 0), groups=G).backward(dz)
    assert np.allclose(dw, w.grad.numpy(), rtol=0, atol=1e-11 * max(1.0, float(w.grad.abs().max())))
    if want_db:
        assert np.allclose(db, dz.sum((0, 2, 3)).numpy(), rtol=0, atol=1e-11 * max(1.0, float(dz.abs().sum())))


# ---- the module ----
@pytest.mark.parametrize("pname", ["reduced", "v1"])
def test_construction_names_shapes_and_round_trip(fixture, pname):
    torch.manual_seed(1)
    m = T.TrainableDiscriminator(**DO.PARAMS[pname])
    ref = D.Discriminator(**DO.PARAMS[pname])
    assert [k for k, _ in m.named_parameters()] == ref.state_dict_keys() == list(m.state_dict()) == m.state_dict_keys()
    names = [str(k) for k in fixture[f"{pname}_names"]]
    shapes = {k: tuple(int(v) for v in row if v) for k, row in zip(names, fixture[f"{pname}_shapes"])}
    assert sorted(names) == sorted(ref.state_dict_keys())
    assert {k: tuple(q.shape) for k, q in m.named_parameters()} == shapes
    for k, q in m.named_parameters():                      # torch's conv initialisation, and weight_norm's g = ||v||
        assert q.requires_grad and q.dtype == torch.float32 and bool(torch.isfinite(q).all())
        if k.endswith(".weight_g"):
            v = m.get_parameter(k[:-1] + "v")
            assert q.shape == (v.shape[0], 1, 1, 1) and v.dim() == 4 and v.shape[3] == 1
            assert torch.equal(q, torch.linalg.vector_norm(v, 2, dim=(1, 2, 3), keepdim=True))
    ref.load_state_dict(m.state_dict())                    # a fresh module's weights go into the eval path
    sd = DO.state_dict(pname)
    m.load_state_dict(sd)                                  # and the reference's checkpoint dict into the module
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    ref.load_state_dict(m.state_dict())
    for (L, w, _), L2 in zip(ref._host, m._descs):
        assert L is not None and L.key == L2.key and tuple(w.shape) == L.weight_shape


def test_plain_period_weights_and_spectral_norm():
    plain = dict(DO.REDUCED, period_discriminator_params=dict(DO.REDUCED["period_discriminator_params"], use_weight_norm=False))
    m = T.TrainableDiscriminator(**plain)
    assert [k for k, _ in m.named_parameters()] == D.Discriminator(**plain).state_dict_keys()
    assert not any(k.endswith(("weight_g", "weight_v")) for k, _ in m.named_parameters())
    assert m.get_parameter("mpd.discriminators.0.convs.0.0.conv.weight").dim() == 4
    spectral = dict(DO.REDUCED, period_discriminator_params=dict(DO.REDUCED["period_discriminator_params"], use_weight_norm=False,
                                                                 use_spectral_norm=True))
    with pytest.raises(NotImplementedError, match="spectral"):
        T.TrainableDiscriminator(**spectral)
    sd = dict(DO.state_dict("reduced"))
    k = "mpd.discriminators.0.convs.0.0.conv"
    sd[f"{k}.weight_orig"], sd[f"{k}.weight_u"] = sd.pop(f"{k}.weight_v"), sd.pop(f"{k}.weight_g")
    with pytest.raises(NotImplementedError, match="spectral"):
        T.TrainableDiscriminator(**DO.REDUCED).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="Missing key"):
        T.TrainableDiscriminator(**DO.REDUCED).load_state_dict({k: v for k, v in DO.state_dict("reduced").items() if "msd" in k})
    with pytest.raises(NotImplementedError, match="LeakyReLU"):
        T.TrainableDiscriminator(**dict(DO.REDUCED, scale_discriminator_params=dict(DO.REDUCED["scale_discriminator_params"],
                                                                                    nonlinear_activation="ReLU")))


def test_loss_arguments():
    with pytest.raises(AssertionError, match="not supported"):
        T.DiscriminatorAdversarialLoss(loss_type="bce")
    crit = T.DiscriminatorAdversarialLoss()
    assert crit.average_by_discriminators is True and crit.loss_type == "mse"


@pytest.mark.parametrize("shape", [(6, 3, 5, 1), (1, 4, 2, 1), (16, 1, 5, 1)])
def test_weight_norm_composition_matches_torch(shape):
    rng = np.random.default_rng(list(shape))
    v = torch.from_numpy(rng.standard_normal(shape))
    g = torch.from_numpy(rng.uniform(0.5, 2.0, (shape[0], 1, 1, 1)))
    up = torch.from_numpy(rng.standard_normal(shape))
    conv = torch.nn.Conv2d(shape[1], shape[0], (shape[2], 1)).double()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        conv = torch.nn.utils.weight_norm(conv)
    with torch.no_grad():
        conv.weight_g.copy_(g)
        conv.weight_v.copy_(v)
    x = torch.from_numpy(rng.standard_normal((2, shape[1], shape[2] + 3, 2)))
    conv(x)                                                # the pre-hook composes conv.weight
    conv.weight.backward(up)
    gl, vl = g.clone().requires_grad_(True), v.clone().requires_grad_(True)
    w = T.weight_norm(gl, vl)
    assert torch.equal(w.detach(), conv.weight.detach())
    w.backward(up)
    assert torch.allclose(gl.grad, conv.weight_g.grad, rtol=1e-13, atol=0) and torch.allclose(vl.grad, conv.weight_v.grad, rtol=1e-12, atol=1e-15)


# ---- the fixture ----
def test_fixture_size_and_caps(golden_dir, fixture):
    assert os.path.getsize(os.path.join(golden_dir, "disc_train.npz")) < (1 << 20)
    for case, (pname, _) in TO.CASES.items():
        names = [str(k) for k in fixture[f"{pname}_names"]]
        sizes = [int(np.prod([v for v in row if v])) for row in fixture[f"{pname}_shapes"]]
        stored = sum(len(TO.param_index(n, pname == "reduced")) for n in sizes)
        for flags in TO.FLAGS:
            eref, gmax, grad = (fixture[f"{case}_{flags}_{what}"] for what in ("eref", "gmax", "grad"))
            assert eref.shape == gmax.shape == (len(names),) and grad.shape == (stored,) and grad.dtype == np.float32
            assert np.all(gmax > 0) and np.all(4 * eref + 1e-6 * gmax <= 5e-5 * gmax), (case, flags)
            i, worst = 0, 0.0
            for n, e, g in zip(sizes, eref, gmax):         # the stored float32 gradient is within its own E_ref of a gradient of size gmax
                part = grad[i:i + len(TO.param_index(n, pname == "reduced"))]
                i += len(part)
                assert float(np.max(np.abs(part))) <= g + e
                worst = max(worst, e / g)
            print(f"{case} {flags}: worst E_ref / gmax {worst:.3g}")
