"""CPU: the trainable vocoder -- host side, and what tests/golden/vocoder_train_*.npz mean.

  * the seven adk_voc_* calls and the plan are in the header, exported and bound, and their argument checks (groups included) run
    on the host before any HIP call; the existing entry points still refuse act = 2;
  * adk_voc_conv_wgrad_plan's grouped slice rule restated and compared;
  * a NumPy walk of the grouped index maps -- which dy row, x channel, packed-weight row and workspace row a (group, row, column)
    touches, forward, backward to the input and weight gradient -- against torch's f64 autograd of F.conv1d(groups=G);
  * TrainableVocoder's construction, naming and loading for the v1, v0, noaddl and use_weight_norm=False parameter sets;
  * the torch weight-norm composition's g / v gradients against torch.nn.utils.weight_norm in f64;
  * the fixtures: their size and the stored caps hold.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_forward_golden as MFG
import make_vocoder_train_golden as MVG
from audiodec_amd import arch, configs, synth
from audiodec_amd import vocoder_train as VT

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("adk_voc_conv", "adk_voc_conv_grad", "adk_voc_convtr", "adk_voc_convtr_grad", "adk_voc_conv_wgrad_plan",
       "adk_voc_conv_wgrad", "adk_voc_convtr_wgrad")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


# ---- the C ABI ----
def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    # the calls are additions: the ABI version every other suite pins is unchanged
    assert f"#define ADK_ABI_VERSION {native.ABI_VERSION}" in header and lib.adk_abi_version() == native.ABI_VERSION


def test_argument_validation_without_device(lib):
    dummy, odd, four = C.c_void_p(16), C.c_void_p(18), C.c_void_p(20)   # never dereferenced: every call fails before a launch
    f = C.c_float

    def conv(x=dummy, w=dummy, bias=dummy, res=dummy, y=dummy, n=2, cin=12, t=100, cout=24, k=11, d=3, g=3, act=2, alpha=0.1, impl=2):
        return lib.adk_voc_conv(x, w, bias, res, y, n, cin, t, cout, k, d, g, act, f(alpha), impl, None)

    def conv_grad(dy=dummy, x=dummy, w=dummy, dres=dummy, dx=dummy, n=2, cin=12, t=100, cout=24, k=11, d=3, g=3, act=2, alpha=0.1):
        return lib.adk_voc_conv_grad(dy, x, w, dres, dx, n, cin, t, cout, k, d, g, act, f(alpha), None)

    def convtr(x=dummy, w=dummy, bias=dummy, y=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=2, alpha=0.1):
        return lib.adk_voc_convtr(x, w, bias, y, n, cin, t, cout, k, s, act, f(alpha), None)

    def convtr_grad(dy=dummy, x=dummy, w=dummy, dx=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=2, alpha=0.1):
        return lib.adk_voc_convtr_grad(dy, x, w, dx, n, cin, t, cout, k, s, act, f(alpha), None)

    def wgrad(dy=dummy, x=dummy, dw=dummy, db=dummy, ws=dummy, n=2, cin=12, t=100, cout=24, k=11, d=3, g=3, act=2, alpha=0.1):
        return lib.adk_voc_conv_wgrad(dy, x, dw, db, ws, n, cin, t, cout, k, d, g, act, f(alpha), None)

    def plan(n=2, cin=12, t=100, cout=24, k=11, d=3, g=3):
        return lib.adk_voc_conv_wgrad_plan(n, cin, t, cout, k, d, g, None, None)

    def twgrad(dy=dummy, x=dummy, dw=dummy, db=dummy, ws=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=2, alpha=0.1):
        return lib.adk_voc_convtr_wgrad(dy, x, dw, db, ws, n, cin, t, cout, k, s, act, f(alpha), None)

    bad_shape = ({"n": -1}, {"cin": 0}, {"t": 0}, {"cout": 0}, {"k": 0}, {"t": -5})
    bad_act = ({"act": 3}, {"act": -1}, {"alpha": float("nan")}, {"act": 1, "alpha": float("nan")})
    bad_groups = ({"g": 0}, {"g": -1}, {"g": 5}, {"g": 4, "cin": 12, "cout": 26}, {"g": 8, "cin": 12, "cout": 24})
    # stride-1 calls: shapes, dilation, groups, activation
    for name, fn in (("adk_voc_conv", conv), ("adk_voc_conv_grad", conv_grad), ("adk_voc_conv_wgrad", wgrad),
                     ("adk_voc_conv_wgrad_plan", plan)):
        for kw in bad_shape + ({"d": 0},) + bad_groups:
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        assert fn(g=5) == ADK_ERR_ARG and b"groups" in lib.adk_last_error(), name
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(n=1 << 20, t=1 << 20) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        # the whole layer's extents, however many groups share them
        assert fn(cin=3 << 28, g=3) == ADK_ERR_ARG and fn(cout=3 << 28, g=3) == ADK_ERR_ARG and fn(d=1 << 29) == ADK_ERR_ARG, name
        if fn is not plan:
            for kw in bad_act:
                assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
    assert wgrad(g=1 << 17, cin=1 << 17, cout=1 << 17, k=1, t=1, n=1) == ADK_ERR_ARG and b"too large" in lib.adk_last_error()
    # transposed calls
    for name, fn in (("adk_voc_convtr", convtr), ("adk_voc_convtr_grad", convtr_grad), ("adk_voc_convtr_wgrad", twgrad)):
        for kw in bad_shape + ({"s": 0}, {"s": -1}) + bad_act:
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        for kw in ({"k": 7}, {"k": 3}, {"k": 6, "s": 2}):
            assert fn(**kw) == ADK_ERR_ARG and b"2 * stride" in lib.adk_last_error(), (name, kw)
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
    assert twgrad(k=38, s=19) == ADK_ERR_ARG and b"too large" in lib.adk_last_error()          # the staging registers' bound
    assert twgrad(ws=four) == ADK_ERR_ARG and b"8-byte aligned" in lib.adk_last_error()
    # impl: 1 or 2, and the direct kernel takes one group only
    assert conv(impl=0) == ADK_ERR_ARG and conv(impl=3) == ADK_ERR_ARG and b"impl" in lib.adk_last_error()
    assert conv(impl=1, g=3) == ADK_ERR_ARG and b"one group" in lib.adk_last_error()
    # pointers: required ones, x only behind an activation, alignment of all
    for fn, needed, optional in ((conv, ("x", "w", "y"), ("bias", "res")), (conv_grad, ("dy", "x", "w", "dx"), ("dres",)),
                                 (convtr, ("x", "w", "y"), ("bias",)), (convtr_grad, ("dy", "x", "w", "dx"), ()),
                                 (wgrad, ("dy", "x", "dw", "ws"), ("db",)), (twgrad, ("dy", "x", "dw", "ws"), ("db",))):
        for p in needed:
            assert fn(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), (fn.__name__, p)
        for p in needed + optional:
            assert fn(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), (fn.__name__, p)
    for fn in (conv_grad, convtr_grad):
        assert fn(x=None, act=1, alpha=1.0) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error()
        assert fn(x=None, act=0, n=0) == 0
    # n_items == 0: a no-op for forward and backward (no pointer is needed), zeros for the weight gradients (dw is needed)
    assert conv(n=0, x=None, w=None, bias=None, res=None, y=None) == 0 and convtr(n=0, x=None, w=None, bias=None, y=None) == 0
    assert conv_grad(n=0, dy=None, x=None, w=None, dres=None, dx=None) == 0
    assert wgrad(n=0, dy=None, x=None, dw=None) == ADK_ERR_ARG and twgrad(n=0, dy=None, x=None, dw=None) == ADK_ERR_ARG
    assert plan() == 0 and plan(n=0) == 0 and plan(g=1) == 0


def test_existing_entry_points_still_refuse_leaky(lib):
    dummy, f = C.c_void_p(16), C.c_float
    calls = {
        "adk_dec_conv": lambda act: lib.adk_dec_conv(dummy, dummy, dummy, dummy, dummy, 2, 8, 100, 16, 7, 3, act, f(0.1), 2, None),
        "adk_dec_conv_grad": lambda act: lib.adk_dec_conv_grad(dummy, dummy, dummy, dummy, dummy, 2, 8, 100, 16, 7, 3, act, f(0.1), None),
        "adk_dec_convtr": lambda act: lib.adk_dec_convtr(dummy, dummy, dummy, dummy, 2, 8, 100, 16, 6, 3, act, f(0.1), None),
        "adk_dec_convtr_grad": lambda act: lib.adk_dec_convtr_grad(dummy, dummy, dummy, dummy, 2, 8, 100, 16, 6, 3, act, f(0.1), None),
        "adk_conv_wgrad": lambda act: lib.adk_conv_wgrad(dummy, dummy, dummy, dummy, dummy, 2, 8, 100, 16, 7, 3, 1, act, f(0.1), None),
        "adk_convtr_wgrad": lambda act: lib.adk_convtr_wgrad(dummy, dummy, dummy, dummy, dummy, 2, 8, 100, 16, 6, 3, act, f(0.1), None),
    }
    for name, call in calls.items():
        assert call(2) == ADK_ERR_ARG and name.encode() in lib.adk_last_error() and b"act must be 0 (none) or 1 (ELU)" in lib.adk_last_error()


# ---- the grouped slice rule ----
def _plan_restated(n, cin, t, cout, k, g):
    cout_g, ck = cout // g, (cin // g) * k
    bm = 128 if cout_g >= 128 else 64 if cout_g >= 64 else 32
    tiles = g * -(-cout_g // bm) * -(-(ck + 1) // 128)
    steps = -(-n * t // 32)
    s0 = max(1, min(-(-512 // tiles), steps // 4))
    per = max(1, -(-steps // s0))
    S = max(1, -(-steps // per))
    return 4 * S * cout * (ck + 1), S, per, steps


@pytest.mark.parametrize("shape", [(16, 768, 160, 768, 11, 3), (16, 384, 800, 384, 11, 3), (16, 96, 9600, 96, 11, 3), (16, 96, 9600, 96, 3, 3),
                                   (16, 256, 160, 256, 7, 1), (2, 15, 51, 15, 11, 3), (3, 99, 33, 99, 3, 3), (1, 21, 400, 36, 11, 3),
                                   (0, 6, 5, 6, 3, 3), (3, 96, 1, 96, 11, 3), (16, 768, 160, 256, 1, 1)])
def test_grouped_wgrad_plan(lib, shape):
    from audiodec_amd import encoder_grad as EG
    n, cin, t, cout, k, g = shape
    ws, S = VT.conv_wgrad_plan(n, cin, t, cout, k, 1, g)
    assert (ws, S) == VT.conv_wgrad_plan(n, cin, t, cout, k, 5, g)           # a function of the shape; the dilation does not enter
    want_ws, want_S, per, steps = _plan_restated(*shape)
    assert (ws, S) == (want_ws, want_S) and 1 <= S <= 512
    assert (S - 1) * per < max(steps, 1)                                       # no slice is empty
    if g == 1:
        assert (ws, S) == EG.wgrad_plan(n, cin, t, cout, k, 1, 1)              # one group: adk_conv_wgrad_plan's


# ---- the grouped index maps ----
@pytest.mark.parametrize("G,cin_g,cout_g,k,d,T", [(3, 2, 2, 3, 1, 7), (3, 2, 3, 11, 5, 51), (3, 3, 2, 11, 5, 13), (2, 1, 2, 7, 3, 20),
                                                  (1, 3, 2, 3, 1, 1), (3, 2, 2, 11, 3, 2)])
def test_grouped_index_maps(G, cin_g, cout_g, k, d, T):
    cin, cout, ck = G * cin_g, G * cout_g, cin_g * k
    rng = np.random.default_rng(1000 * G + 100 * k + 10 * d + T)
    w, x, b = rng.standard_normal((cout, cin_g, k)), rng.standard_normal((cin, T)), rng.standard_normal(cout)
    dy = rng.standard_normal((cout, T))
    xr, wr = torch.from_numpy(x)[None].requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    yr = F.conv1d(F.pad(xr, ((k - 1) * d, 0)), wr, torch.from_numpy(b), dilation=d, groups=G)
    yr.backward(torch.from_numpy(dy)[None])
    pf, pg = VT.pack_conv(torch.from_numpy(w), G).numpy(), VT.pack_conv_grad(torch.from_numpy(w), G).numpy()
    assert pf.shape == (G, ck, cout_g) and pg.shape == (G, cout_g * k, cin_g)
    y, dx = np.full((cout, T), np.nan), np.full((cin, T), np.nan)
    ws = np.full((cout, ck + 1), np.nan)                       # one slice of the workspace: [c_out][ck + 1], all groups' rows
    for g in range(G):                                         # blockIdx.z
        for u in range(T):
            for m in range(cout_g):                            # forward: row m of the group is output channel g cout_g + m
                acc = b[g * cout_g + m]
                for kk in range(ck):
                    ci, j = divmod(kk, k)
                    t = u - (k - 1 - j) * d
                    if t >= 0:
                        acc += pf[g, kk, m] * x[g * cin_g + ci, t]
                assert np.isnan(y[g * cout_g + m, u])
                y[g * cout_g + m, u] = acc
            for m in range(cin_g):                             # backward: row m is input channel g cin_g + m
                acc = 0.0
                for kk in range(cout_g * k):
                    co, j = divmod(kk, k)
                    t = u + (k - 1 - j) * d
                    if t < T:
                        acc += pg[g, kk, m] * dy[g * cout_g + co, t]
                assert np.isnan(dx[g * cin_g + m, u])
                dx[g * cin_g + m, u] = acc
        for m in range(cout_g):                                # weight gradient: dy row and workspace row g cout_g + m
            for n in range(ck + 1):
                if n == ck:
                    v = dy[g * cout_g + m].sum()
                else:
                    ci, j = divmod(n, k)
                    back = (k - 1 - j) * d
                    v = sum(dy[g * cout_g + m, u] * x[g * cin_g + ci, u - back] for u in range(back, T))
                assert np.isnan(ws[g * cout_g + m, n])         # every workspace element is written by exactly one group
                ws[g * cout_g + m, n] = v
    assert np.allclose(y, yr.detach().numpy()[0], rtol=0, atol=1e-12)
    assert np.allclose(dx, xr.grad.numpy()[0], rtol=0, atol=1e-12)
    assert np.allclose(ws[:, :ck].reshape(cout, cin_g, k), wr.grad.numpy(), rtol=0, atol=1e-12)    # the fold's layout is dW's own
    assert np.allclose(ws[:, ck], dy.sum(1), rtol=0, atol=1e-12)
    if G == 1:
        from audiodec_amd import decoder_grad as DG
        assert np.array_equal(pf[0], DG.pack_conv(torch.from_numpy(w)).numpy())
        assert np.array_equal(pg[0], DG.pack_conv_grad(torch.from_numpy(w)).numpy())


# ---- the module: host work ----
def _params(name, **over):
    _, p = MVG.generator_params(name)
    p.update(over)
    return p


def _expected_keys(p):
    exp = {}
    for s in arch.hifigan_convs(p):
        if s.wn:
            exp[s.wkey("weight_g")], exp[s.wkey("weight_v")] = (s.wshape[0], 1, 1), tuple(s.wshape)
        else:
            exp[s.wkey("weight")] = tuple(s.wshape)
        if s.bias:
            exp[s.wkey("bias")] = (s.cout,)
    return exp


@pytest.mark.parametrize("name,n_params", [("v1", 98), ("v0", 234), ("noaddl", 62)])
def test_construction_and_naming(name, n_params):
    p = _params(name)
    voc = VT.TrainableVocoder(**p)
    got = {k: tuple(q.shape) for k, q in voc.named_parameters()}
    assert got == _expected_keys(p) and len(got) == n_params
    assert {k: tuple(v.shape) for k, v in voc.named_buffers()} == {"mean": (64,), "scale": (64,)}
    assert voc.hop == 300 and voc.multigroup == (name != "v0") and voc.additional == (name != "noaddl")
    # weight norm's initial g is ||v||, so the composed weight is v
    g, v = voc.get_parameter("upsamples.0.deconv.weight_g"), voc.get_parameter("upsamples.0.deconv.weight_v")
    assert g.shape == (512, 1, 1) and torch.allclose(VT.weight_norm(g, v), v, rtol=1e-6, atol=0)
    assert 0.005 < float(v.detach().std()) < 0.02                                       # reset_parameters: normal_(0, 0.01)
    # the checkpoint dict loads, its pad_buffer entries ignored, and comes back out
    tag, _ = MVG.generator_params(name)
    sd = synth.synth_state_dict(tag, MFG.SEED)
    assert any(k.endswith(".pad_buffer") for k in sd)
    voc.load_state_dict(sd)
    out = voc.state_dict()
    assert set(out) == {k for k in sd if not k.endswith(".pad_buffer")}
    assert all(torch.equal(out[k], sd[k]) for k in out)
    # and goes back into the streaming generator with the pad buffers the generator expects
    from audiodec_amd.stream_generator import HiFiGANStreamGenerator
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        HiFiGANStreamGenerator(**p).load_state_dict({**sd, **out})
    with pytest.raises(RuntimeError, match="Missing key"):
        voc.load_state_dict({k: v for k, v in sd.items() if k != "output_conv.conv.bias"})
    with pytest.raises(RuntimeError, match="size mismatch"):
        voc.load_state_dict({**sd, "mean": torch.zeros(3)})
    # the activation in front of each conv
    acts = {layer.spec.name: (layer.act, layer.alpha) for layer in voc._layers}
    assert acts["input_conv"] == (0, 0.0) and acts["output_conv"] == (2, pytest.approx(0.01)) and acts["upsamples.2"] == (2, pytest.approx(0.1))
    assert all(a == (0, 0.0) for k, a in acts.items() if k.endswith("conv_out"))
    assert voc._layers[-1].impl == 1 and all(layer.impl == 2 for layer in voc._layers[:-1])


def test_without_weight_norm_and_without_stats():
    p = _params("v1", use_weight_norm=False, stats=None)
    voc = VT.TrainableVocoder(**p)
    got = {k: tuple(q.shape) for k, q in voc.named_parameters()}
    assert got == _expected_keys(p) and "blocks.0.convs1.0.conv.weight" in got and not any("weight_g" in k for k in got)
    assert got["blocks.0.convs1.0.conv.weight"] == (768, 256, 11) and got["blocks.3.conv_out.weight"] == (32, 96, 1)
    assert dict(voc.named_buffers()) == {} and not voc.norm
    assert len(got) == 64


def test_construction_errors():
    with pytest.raises(NotImplementedError, match="LeakyReLU"):
        VT.TrainableVocoder(nonlinear_activation="ELU", nonlinear_activation_params={})
    with pytest.raises(NotImplementedError, match="negative_slope"):
        VT.TrainableVocoder(nonlinear_activation_params={"negative_slope": 0.1, "inplace": True})
    with pytest.raises(NotImplementedError, match="2 \\* scale"):
        VT.TrainableVocoder(upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 5))
    with pytest.raises(AssertionError):
        VT.TrainableVocoder(kernel_size=6)
    with pytest.raises(AssertionError):
        VT.TrainableVocoder(upsample_scales=(8, 8, 2), upsample_kernel_sizes=(16, 16, 4, 4))
    with pytest.raises(AssertionError):
        VT.TrainableVocoder(resblock_kernel_sizes=(3, 7))
    with pytest.raises(TypeError, match="unexpected keyword"):
        VT.TrainableVocoder(hop=300)
    with pytest.raises(ValueError, match="positive"):
        VT.TrainableVocoder(channels=8)
    from audiodec_amd.stream_generator import HiFiGANStreamGenerator
    with pytest.raises(RuntimeError, match="no weights loaded"):
        VT.TrainableVocoder.from_generator(HiFiGANStreamGenerator(**_params("v1")))
    voc = VT.TrainableVocoder(**_params("noaddl"))
    for bad in (torch.zeros(2, 63, 5), torch.zeros(64, 5), torch.zeros(0, 64, 5), torch.zeros(2, 64, 0), None):
        with pytest.raises(ValueError, match="expected a|empty input"):
            voc(bad)


def test_from_generator_copies_the_loaded_weights():
    from audiodec_amd.stream_generator import HiFiGANStreamGenerator
    tag, p = MVG.generator_params("noaddl")
    sd = synth.synth_state_dict(tag, MFG.SEED)
    gen = HiFiGANStreamGenerator(**p)
    gen.load_state_dict(sd)
    voc = VT.TrainableVocoder.from_generator(gen)
    assert all(torch.equal(v, sd[k]) for k, v in voc.state_dict().items())
    assert torch.equal(voc.mean, sd["mean"]) and torch.equal(voc.scale, sd["scale"])


def test_saved_floats_counts_every_conv_input_once():
    for name in ("v1", "v0", "noaddl"):
        voc = VT.TrainableVocoder(**_params(name))
        B, T = 2, 7
        t, n, specs = T, 0, voc._specs
        lengths = []
        for s in specs:
            lengths.append(t)
            t *= s.stride if s.kind == "convT" else 1
        n = sum(B * s.cin * tt for s, tt in zip(specs, lengths))
        if name == "v0":        # the three chains of a stage start from one tensor: two of the three first convs' inputs are shared
            n -= sum(2 * B * s.cin * tt for s, tt in zip(specs, lengths) if s.name.endswith("blocks.0.convs1.0"))
        assert voc.saved_floats(B, T) == n + B * 1 * T * 300, name


# ---- weight norm in torch ----
@pytest.mark.parametrize("shape", [(6, 4, 11), (5, 7, 10), (3, 9, 1)])
def test_weight_norm_composition_matches_torch(shape):
    rng = np.random.default_rng(sum(shape))
    v0 = torch.from_numpy(rng.standard_normal(shape))
    g0 = torch.from_numpy(rng.standard_normal((shape[0], 1, 1)))
    up = torch.from_numpy(rng.standard_normal(shape))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = torch.nn.utils.weight_norm(torch.nn.Conv1d(shape[1], shape[0], shape[2], bias=False).double())
    with torch.no_grad():
        m.weight_g.copy_(g0)
        m.weight_v.copy_(v0)
    m(torch.zeros(1, shape[1], shape[2], dtype=torch.float64))                  # the pre-forward hook composes m.weight
    (m.weight * up).sum().backward()
    g, v = g0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    w = VT.weight_norm(g, v)
    (w * up).sum().backward()
    assert torch.allclose(w, m.weight, rtol=1e-13, atol=0)
    assert torch.allclose(g.grad, m.weight_g.grad, rtol=1e-12, atol=1e-13) and torch.allclose(v.grad, m.weight_v.grad, rtol=1e-12, atol=1e-13)


# ---- the fixtures ----
@pytest.mark.parametrize("name,n_params", [("v1", 98), ("v0", 234), ("noaddl", 62)])
def test_fixture_size_and_caps(golden_dir, name, n_params):
    path = os.path.join(golden_dir, f"vocoder_train_{name}.npz")
    assert os.path.getsize(path) < (1 << 20)
    fx = np.load(path, allow_pickle=False)
    names = [str(k) for k in fx["names"]]
    assert len(names) == n_params and set(names) == set(_expected_keys(_params(name)))
    assert fx["y64"].shape == (2, 1, 2100) and fx["gc64"].shape == (2, 64, 7) and int(fx["seed"]) == 5
    mx, er = fx["max"], fx["E_ref"]
    assert mx.shape == er.shape == (2 + n_params,)
    assert np.all(4 * er + 1e-6 * mx <= MVG.CAP * mx)                           # the project's cap, tensor by tensor
    assert mx[2:].min() >= 0.25                                                 # a dropped tap or group cannot hide under the bound
    exp = _expected_keys(_params(name))
    for i, k in enumerate(names):
        size = int(np.prod(exp[k]))
        assert fx[f"g{i}"].shape == ((size,) if size <= MVG.WHOLE else (-(-size // MVG.STEP),)), k
        assert np.abs(fx[f"g{i}"]).max() <= mx[2 + i]
    # the sampling stride is prime to every kernel size and channel count
    assert all(np.gcd(MVG.STEP, v) == 1 for v in (3, 7, 11, 10, 8, 6, 32, 64, 96, 128, 192, 256, 384, 512, 768))
    assert np.array_equal(MVG.case_input(), np.load(os.path.join(golden_dir, "forward.npz"))["b3_zq"][:2, :, :7])
