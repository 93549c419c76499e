"""CPU: the trainable decoder -- host side, and what tests/golden/decoder_train.npz means.

  * a NumPy walk of adk_convtr_wgrad's index map -- the GEMM's columns n = co 2s + q, the operand g, and the staging that scatters
    each dy element of a 33-frame run to its two slots -- against torch's f64 autograd of a restated replicate-pad /
    conv_transpose1d / crop;
  * adk_convtr_wgrad_plan and adk_convtr_wgrad are in the header, exported and bound, the ABI is 14, and their argument checks run
    on the host before any HIP call; the plan's slice rule restated and compared;
  * TrainableDecoder's construction, naming and loading in both key styles are host work; the merged state dict loads into the
    streaming generator;
  * the fixture: its size and the stored caps hold.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_decoder_train_golden as MTG
import make_forward_golden as MFG
from audiodec_amd import decoder_grad as DG
from audiodec_amd import decoder_train as DT
from audiodec_amd import synth

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("adk_convtr_wgrad_plan", "adk_convtr_wgrad")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "decoder_train.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def convtr_ref(x, w, b, s):
    """CausalConvTranspose1d.forward (layers/conv_layer.py:189-192) for kernel 2s in torch ops: replicate padding by one frame,
    the transposed conv, one stride cropped at both ends."""
    y = F.conv_transpose1d(F.pad(x, (1, 0), mode="replicate"), w, b, stride=s)
    return y[:, :, s:-s]


# ---- the index map ----
def _g(dy, b, co, i, q, s):
    """The GEMM's B operand: dy (B, C_out, T s)."""
    ts = dy.shape[2]
    v = dy[b, co, i * s + q] if i * s + q < ts else 0.0
    if i == 0 and q >= s:
        v += dy[b, co, q - s]
    return v


def _walk_direct(dy, x, s):
    """dW[ci][co][q] = sum_{b,i} x[b][ci][i] g(b, co, i, q) and db[co] = sum dy, term by term."""
    B, cin, T = x.shape
    cout = dy.shape[1]
    dw = np.zeros((cin, cout * 2 * s))
    for b in range(B):
        for i in range(T):
            for n in range(cout * 2 * s):
                co, q = divmod(n, 2 * s)
                dw[:, n] += x[b, :, i] * _g(dy, b, co, i, q, s)
    return dw.reshape(cin, cout, 2 * s), dy.sum((0, 2))


def _walk_staged(dy, x, s, depth=32):
    """The same sum the way convtr_wgrad_kernel stages it: per 32-deep step and channel, the elements (frame f of the 33-frame run,
    phase j) each go to column j of row f and to column s + j of row f - 1; the second slot takes the element when both rows are in
    one item, plus the padding's share dy[b][co][j] when its own row is a frame 0.  Every slot is written exactly once."""
    B, cin, T = x.shape
    cout, red = dy.shape[1], B * T
    dw = np.zeros((cin, cout * 2 * s))
    for rho0 in range(0, red, depth):
        a = np.zeros((depth, cin))
        for r in range(depth):
            if rho0 + r < red:
                a[r] = x[(rho0 + r) // T, :, (rho0 + r) % T]
        bs = np.full((depth, cout * 2 * s), np.nan)
        for co in range(cout):
            for f in range(depth + 1):
                for j in range(s):
                    rho = rho0 + f
                    live = rho < red
                    item, fr = (rho // T, rho % T) if live else (0, 0)
                    val = dy[item, co, fr * s + j] if live else 0.0
                    if f < depth:
                        assert np.isnan(bs[f, co * 2 * s + j])
                        bs[f, co * 2 * s + j] = val
                    if f >= 1:
                        inside = live and fr >= 1
                        t_live = rho - 1 < red
                        t_item = item if inside else item - 1 if live else B - 1
                        t_f = fr - 1 if inside else T - 1
                        v = (val if inside else 0.0) + (dy[t_item, co, j] if t_live and t_f == 0 else 0.0)
                        assert np.isnan(bs[f - 1, co * 2 * s + s + j])
                        bs[f - 1, co * 2 * s + s + j] = v if t_live else 0.0
        assert not np.isnan(bs).any()
        for r in range(depth):                                              # the slots hold g
            if rho0 + r < red:
                b, i = divmod(rho0 + r, T)
                want = [_g(dy, b, n // (2 * s), i, n % (2 * s), s) for n in range(cout * 2 * s)]
                assert np.array_equal(bs[r], np.asarray(want))
            else:
                assert not bs[r].any()
        dw += a.T @ bs
    return dw.reshape(cin, cout, 2 * s)


@pytest.mark.parametrize("T", [1, 2, 3, 33])
@pytest.mark.parametrize("s", [3, 4, 5])
def test_convtr_wgrad_index_map(s, T):
    B, cin, cout = 3, 3, 2
    rng = np.random.default_rng(100 * s + T)
    x, w, b = rng.standard_normal((B, cin, T)), rng.standard_normal((cin, cout, 2 * s)), rng.standard_normal(cout)
    dy = rng.standard_normal((B, cout, T * s))
    xr, wr, br = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    y = convtr_ref(xr, wr, br, s)
    assert tuple(y.shape) == dy.shape
    y.backward(torch.from_numpy(dy))
    dw, db = _walk_direct(dy, x, s)
    assert np.allclose(dw, wr.grad.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(db, br.grad.numpy(), rtol=0, atol=1e-12)
    for depth in (32, 4):                                                   # 4: steps that start and end inside items
        assert np.allclose(_walk_staged(dy, x, s, depth), wr.grad.numpy(), rtol=0, atol=1e-12)
    # the forward the kernels implement is the reference's layer
    yk = np.zeros_like(dy)
    for i in range(T):
        for r in range(s):
            yk[:, :, i * s + r] = b + np.einsum("bc,co->bo", x[:, :, i], w[:, :, r]) + \
                np.einsum("bc,co->bo", x[:, :, max(i - 1, 0)], w[:, :, s + r])
    assert np.allclose(yk, y.detach().numpy(), rtol=0, atol=1e-12)


# ---- the C ABI ----
def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd, four = C.c_void_p(16), C.c_void_p(18), C.c_void_p(20)   # never dereferenced: every call fails before a launch

    def wgrad(dy=dummy, x=dummy, dw=dummy, db=dummy, ws=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=1, alpha=1.0):
        return lib.adk_convtr_wgrad(dy, x, dw, db, ws, n, cin, t, cout, k, s, act, C.c_float(alpha), None)

    def plan(n=2, cin=8, t=100, cout=16, k=6, s=3):
        return lib.adk_convtr_wgrad_plan(n, cin, t, cout, k, s, None, None)

    for name, fn in (("adk_convtr_wgrad", wgrad), ("adk_convtr_wgrad_plan", plan)):
        for kw in ({"n": -1}, {"cin": 0}, {"t": 0}, {"cout": 0}, {"k": 0}, {"s": 0}, {"s": -1}, {"t": -5}):
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        for kw in ({"k": 7}, {"k": 3}, {"k": 6, "s": 2}):
            assert fn(**kw) == ADK_ERR_ARG and b"2 * stride" in lib.adk_last_error(), (name, kw)
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(n=1 << 16, t=1 << 16) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(cin=1 << 28) == ADK_ERR_ARG and fn(cout=1 << 28) == ADK_ERR_ARG, name
        assert fn(k=140000, s=70000) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(k=38, s=19) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name    # the staging registers' bound
    assert plan(k=36, s=18) == 0 and plan() == 0 and plan(n=0) == 0
    for kw in ({"act": 2}, {"act": -1}, {"alpha": float("nan")}):
        assert wgrad(**kw) == ADK_ERR_ARG and b"adk_convtr_wgrad" in lib.adk_last_error(), kw
    for p in ("dy", "x", "dw", "ws"):
        assert wgrad(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), p
    for p in ("dy", "x", "dw", "db", "ws"):
        assert wgrad(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), p
    assert wgrad(ws=four) == ADK_ERR_ARG and b"8-byte aligned" in lib.adk_last_error()     # the f64 slab behind the partials
    assert wgrad(n=0, dy=None, x=None, dw=None) == ADK_ERR_ARG                             # n_items == 0 still writes dw


# ---- the slice rule ----
def _plan_restated(n, cin, t, cout, s):
    bm = 128 if cin >= 128 else 64 if cin >= 64 else 32
    nn = cout * 2 * s
    tiles = -(-cin // bm) * -(-nn // 128)
    steps = -(-n * t // 32)
    s0 = max(1, min(-(-512 // tiles), steps // 4))
    per = max(1, -(-steps // s0))
    S = max(1, -(-steps // per))
    total = n * t * s
    want = max(1, min(64, -(-total // 4096)))
    chunk = max(1, -(-total // want))
    chunks = max(1, -(-total // chunk))
    floats = S * cin * (nn + 1)
    return 4 * (floats + floats % 2) + 8 * chunks * cout, S, per, steps


@pytest.mark.parametrize("shape", [(16, 512, 160, 256, 5), (16, 256, 800, 128, 5), (16, 128, 4000, 64, 4), (16, 64, 16000, 32, 3),
                                   (2, 64, 11, 32, 3), (3, 512, 1, 256, 5), (0, 64, 5, 32, 3), (1, 33, 101, 5, 4), (3, 136, 5, 128, 5),
                                   (1, 8, 4000, 4, 3)])
def test_convtr_wgrad_plan(lib, shape):
    n, cin, t, cout, s = shape
    ws, S = DT.convtr_wgrad_plan(n, cin, t, cout, 2 * s, s)
    assert (ws, S) == DT.convtr_wgrad_plan(n, cin, t, cout, 2 * s, s)     # a function of the shape
    want_ws, want_S, per, steps = _plan_restated(n, cin, t, cout, s)
    assert (ws, S) == (want_ws, want_S) and 1 <= S <= 512
    assert (S - 1) * per < max(steps, 1)                                    # no slice is empty
    assert ws % 8 == 0


def test_convtr_wgrad_plan_splits_a_long_reduction(lib):
    assert DT.convtr_wgrad_plan(1, 8, 4000, 4, 6, 3)[1] >= 3 and DT.convtr_wgrad_plan(1, 8, 16, 4, 6, 3)[1] == 1


# ---- host side of TrainableDecoder ----
def test_construction_and_shape_errors_without_device():
    with pytest.raises(NotImplementedError, match="weight_g"):
        DT.TrainableDecoder(use_weight_norm=True)
    with pytest.raises(NotImplementedError, match="causal"):
        DT.TrainableDecoder(mode="noncausal")
    with pytest.raises(NotImplementedError, match="ELU"):
        DT.TrainableDecoder(nonlinear_activation="LeakyReLU")
    with pytest.raises(NotImplementedError, match="alpha"):
        DT.TrainableDecoder(nonlinear_activation_params={"inplace": True})
    with pytest.raises(NotImplementedError, match="ActivateDecoder"):
        DT.TrainableDecoder(codec="activate_audiodec")
    with pytest.raises(NotImplementedError, match="written for 7"):
        DT.TrainableDecoder(kernel_size=5)
    with pytest.raises(ValueError, match="same length"):
        DT.TrainableDecoder(dec_ratios=(8, 4, 2), dec_strides=(5, 5, 4, 3))
    with pytest.raises(ValueError, match="positive"):
        DT.TrainableDecoder(dec_strides=(5, 5, 0, 3))
    with pytest.raises(ValueError, match="positive"):
        DT.TrainableDecoder(code_dim=0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        DT.TrainableDecoder(channels=3)
    dec = DT.TrainableDecoder(kernel_size=7)
    assert dec.hop == 300 and dec.code_dim == 64 and dec.output_channels == 1
    assert all(p.device.type == "cpu" and p.dtype == torch.float32 and p.requires_grad for p in dec.parameters())
    for bad in (torch.zeros(1, 2, 30), torch.zeros(1, 30), torch.zeros(1, 64, 30, 1), torch.zeros(0, 64, 30), torch.zeros(1, 64, 0)):
        with pytest.raises(ValueError, match="expected a|empty input"):
            dec(bad)
    # what a differentiable pass keeps: the input of every conv -- conv1's, per block the transposed conv's and six residual-unit
    # convs', conv2's
    c_in, c, t_in, t_out = [512, 256, 128, 64], [256, 128, 64, 32], [1, 5, 25, 100], [5, 25, 100, 300]
    want = 64 + sum(ci * ti + 6 * co * to for ci, co, ti, to in zip(c_in, c, t_in, t_out)) + 32 * 300
    assert dec.saved_floats(1, 1) == want
    assert dec.saved_floats(2, 11) == 2 * 11 * want
    frozen = DG.FrozenDecoder(64, 1, 32)
    assert dec.saved_floats(1, 1) > frozen.saved_floats(1, 1)              # the frozen decoder keeps the activated convs' only


def test_parameter_names_and_state_dict(fixture):
    enc_tag, pe = MTG.generator_params("vctk_sym")
    dec = DT.TrainableDecoder(**pe)
    names = [k for k, _ in dec.named_parameters()]
    for case in MTG.CASES:
        assert names == [str(k) for k in fixture[f"{case}_names"]]
    assert len(names) == 34 and names[0] == "decoder.conv1.conv.weight" and names[-1] == "decoder.conv2.conv.weight"
    assert "decoder.conv_blocks.2.res_units.1.conv2.weight" in names and "decoder.conv_blocks.3.conv.deconv.bias" in names
    assert dec.get_parameter("decoder.conv_blocks.0.conv.deconv.weight").shape == (512, 256, 10)
    assert list(dec.state_dict()) == names and names == DG.FrozenDecoder(64, 1, 32).state_dict_keys()
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    assert any(k.startswith("encoder.") for k in sd) and any(k.endswith(".pad_buffer") for k in sd)
    dec.load_state_dict(sd)                                            # the generator's dict: the rest is ignored
    for k, p in dec.named_parameters():
        assert torch.equal(p.detach(), sd[k]) and p.data_ptr() != sd[k].data_ptr()
    # the decoder's own keys, without the prefix (what the reference's decoder.state_dict() holds)
    own = {k[len("decoder."):]: v * 2 for k, v in sd.items() if k.startswith("decoder.")}
    assert any(k.endswith(".pad_buffer") for k in own)
    dec2 = DT.TrainableDecoder(**pe)
    dec2.load_state_dict(own)
    for k, p in dec2.named_parameters():
        assert torch.equal(p.detach(), 2 * sd[k])
    with pytest.raises(RuntimeError, match="Missing key"):
        DT.TrainableDecoder(**pe).load_state_dict({k: v for k, v in sd.items() if k != "decoder.conv2.conv.weight"})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        DT.TrainableDecoder(**pe).load_state_dict(dict(sd, **{"decoder.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        DT.TrainableDecoder(**pe).load_state_dict(dict(sd, **{"decoder.conv2.conv.weight": torch.zeros(2, 32, 7)}))
    # the merged dict loads back into the streaming generator
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    with torch.no_grad():
        dec.get_parameter("decoder.conv_blocks.1.conv.deconv.weight").mul_(2.0)
    gen = AutoEncoderStreamGenerator(**pe)
    gen.load_state_dict({**sd, **dec.state_dict()})
    k = "decoder.conv_blocks.1.conv.deconv.weight"
    assert torch.equal(gen._sd[k], 2.0 * sd[k])
    assert torch.equal(gen._sd["encoder.conv.conv.weight"], sd["encoder.conv.conv.weight"])
    stereo = DT.TrainableDecoder(**MTG.generator_params("test_stereo_sym")[1])
    assert stereo.output_channels == 2 and stereo.get_parameter("decoder.conv2.conv.weight").shape == (2, 32, 7)


def test_packs_follow_the_parameter_version():
    from audiodec_amd import arch
    layer = DT._Layer(arch.ConvSpec("op", "convT", 3, 4, 6, 3, 1, 1, True, False), DG.ACT_NONE, 1.0)
    w = torch.nn.Parameter(torch.randn(3, 4, 6))
    wf, wg = layer.packs(w)
    assert layer.packs(w)[0] is wf and layer.packs(w)[1] is wg         # not rebuilt on every call
    assert torch.equal(wf, DG.pack_convtr(w.detach(), 3)) and torch.equal(wg, DG.pack_convtr_grad(w.detach(), 3))
    assert not wf.requires_grad and not wg.requires_grad
    with torch.no_grad():
        w.add_(1.0)                                                    # what an optimizer step does
    wf2, wg2 = layer.packs(w)
    assert wf2 is not wf and torch.equal(wf2, DG.pack_convtr(w.detach(), 3)) and torch.equal(wg2, DG.pack_convtr_grad(w.detach(), 3))
    direct = DT._Layer(arch.ConvSpec("op", "conv", 32, 1, 7, 1, 1, 1, False, False), DG.ACT_NONE, 1.0)
    w2 = torch.nn.Parameter(torch.randn(1, 32, 7))
    assert direct.impl == DG.IMPL_DIRECT and torch.equal(direct.packs(w2)[0], w2.detach())    # conv2: the reference's layout
    assert torch.equal(direct.packs(w2)[1], DG.pack_conv_grad(w2.detach()))


# ---- the fixture ----
def test_fixture_size(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "decoder_train.npz")) < (1 << 20)


@pytest.mark.parametrize("name", list(MTG.CASES))
def test_fixture_is_consistent(fixture, name):
    model, _, sl = MTG.CASES[name]
    dec = DT.TrainableDecoder(**MTG.generator_params(model)[1])
    assert int(fixture[f"{name}_seed"]) == MTG.case_seed(name) and tuple(fixture[f"{name}_slice"]) == sl
    zq = MTG.case_input(name)
    shape = (sl[1] - sl[0], 64, sl[3] - sl[2])
    assert zq.shape == shape and zq.dtype == np.float32
    y64, gzq64 = fixture[f"{name}_y64"], fixture[f"{name}_gzq64"]
    assert y64.dtype == np.float64 and y64.shape == (shape[0], dec.output_channels, shape[2] * dec.hop) and gzq64.shape == shape
    names = [str(k) for k in fixture[f"{name}_names"]]
    mx, er = fixture[f"{name}_max"], fixture[f"{name}_E_ref"]
    assert len(names) == 34 and len(mx) == len(er) == len(names) + 2
    assert mx[0] == np.abs(y64).max() and mx[1] == np.abs(gzq64).max()
    for i, (k, p) in enumerate(dec.named_parameters()):
        g = fixture[f"{name}_g{i}"]
        assert g.dtype == np.float64 and g.shape == MTG.sample(np.empty(p.numel())).shape and np.isfinite(g).all()
        assert 0 < np.abs(g).max() <= mx[i + 2]
    for e, m in zip(er, mx):
        assert 0 < e and 4 * e + 1e-6 * m <= MTG.CAP * m                # the cap: the bound cannot hide a dropped tap
    # the decoder-grad fixture's answers for the same cases (two f64 runs: they differ by the order of f64 sums at most)
    old = np.load(os.path.join(os.path.dirname(MTG.OUT), "decoder_grad.npz"), allow_pickle=False)
    assert np.allclose(old[f"{name}_y64"], y64, rtol=1e-9, atol=1e-12) and np.allclose(old[f"{name}_grad64"], gzq64, rtol=1e-9, atol=1e-12)
