"""CPU: the trainable encoder -- host side, and what tests/golden/encoder_grad.npz means.

  * NumPy walks of the strided conv's forward GEMM, of its phase-split backward (pack_down_grad) and of the weight gradient's
    index map, the way the kernels walk them, against torch's f64 conv and its autograd;
  * adk_enc_down, adk_enc_down_grad, adk_conv_wgrad_plan and adk_conv_wgrad are in the header, exported and bound, the ABI is 14,
    and their argument checks run on the host before any HIP call;
  * adk_conv_wgrad_plan: deterministic, S >= 1, the workspace covers S partial tiles, a long reduction is split;
  * TrainableEncoder's construction, loading and shape errors are raised before any device is touched; its parameter names are
    the reference's;
  * the fixture: the stored caps hold.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_encoder_grad_golden as MEG
import make_forward_golden as MFG
from audiodec_amd import decoder_grad as DG
from audiodec_amd import encoder_grad as EG
from audiodec_amd import synth

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("adk_enc_down", "adk_enc_down_grad", "adk_conv_wgrad_plan", "adk_conv_wgrad")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "encoder_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def _torch_conv(x, w, k, d, s):
    """CausalConv1d.forward (layers/conv_layer.py:146-149) on (C, T) f64 arrays, with autograd."""
    xr = torch.from_numpy(x)[None].requires_grad_(True)
    wr = torch.from_numpy(w).requires_grad_(True)
    return xr, wr, F.conv1d(F.pad(xr, ((k - 1) * d, 0)), wr, stride=s, dilation=d)


# ---- index maps ----
@pytest.mark.parametrize("s", [3, 4, 5])
def test_down_packings(s):
    k, cin, cout = 2 * s, 3, 4
    for T in (1, s - 1, s, s + 1, 2 * s + 1):
        rng = np.random.default_rng(100 * s + T)
        w, x = rng.standard_normal((cout, cin, k)), rng.standard_normal((cin, T))
        t_out = EG.out_length(T, s)
        dy = rng.standard_normal((cout, t_out))
        pf, pg = DG.pack_conv(torch.from_numpy(w)).numpy(), EG.pack_down_grad(torch.from_numpy(w), s).numpy()
        assert pf.shape == (cin * k, cout) and pg.shape == (s, 2 * cout, cin)
        y, dx = np.zeros((cout, t_out)), np.full((cin, T), np.nan)
        for u in range(t_out):                                     # forward GEMM: kk = ci k + j reads x[ci][u s - (k-1-j)]
            for kk in range(cin * k):
                ci, j = divmod(kk, k)
                t = u * s - (k - 1 - j)
                assert t < T
                if t >= 0:
                    y[:, u] += pf[kk] * x[ci, t]
        for r in range(s):                                         # backward: one GEMM per phase, kk = 2 co + tap
            cnt = len(range(r, T, s))
            for q in range(cnt):
                acc = np.zeros(cin)
                for kk in range(2 * cout):
                    co, tap = divmod(kk, 2)
                    u = q + (2 if r else 1) - tap
                    if u < t_out:
                        acc += pg[r, kk] * dy[co, u]
                assert np.isnan(dx[:, q * s + r]).all()            # every input index is written by exactly one phase
                dx[:, q * s + r] = acc
        xr, _, yr = _torch_conv(x, w, k, 1, s)
        assert tuple(yr.shape) == (1, cout, t_out)
        yr.backward(torch.from_numpy(dy)[None])
        assert np.allclose(y, yr.detach().numpy()[0], rtol=0, atol=1e-12)
        assert np.allclose(dx, xr.grad.numpy()[0], rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="2 \\* stride"):
        EG.pack_down_grad(torch.zeros(2, 2, 2 * s + 1), s)


def _wgrad_walk(dy, x, k, d, s):
    """adk_conv_wgrad's GEMM: n = ci k + j (the last column's tap is 1), reduction over u."""
    cout, t_out = dy.shape
    cin, T = x.shape
    acc = np.zeros((cout, cin * k + 1))
    for u in range(t_out):
        for n in range(cin * k + 1):
            if n == cin * k:
                acc[:, n] += dy[:, u]
                continue
            ci, j = divmod(n, k)
            t = u * s - (k - 1 - j) * d
            assert t < T
            if t >= 0:
                acc[:, n] += dy[:, u] * x[ci, t]
    return acc[:, :-1].reshape(cout, cin, k), acc[:, -1]


WGRAD_WALKS = [(2 * s, 1, s, T) for s in (3, 4, 5) for T in (1, s - 1, s, s + 1, 2 * s + 1)] + \
              [(7, d, 1, 37) for d in (1, 3, 9)] + [(1, 1, 1, 5), (3, 1, 1, 2)]


@pytest.mark.parametrize("k,d,s,T", WGRAD_WALKS)
def test_wgrad_index_map(k, d, s, T):
    cin, cout = 3, 2
    rng = np.random.default_rng(1000 * k + 100 * d + 10 * s + T)
    w, x = rng.standard_normal((cout, cin, k)), rng.standard_normal((cin, T))
    dy = rng.standard_normal((cout, EG.out_length(T, s)))
    _, wr, yr = _torch_conv(x, w, k, d, s)
    assert tuple(yr.shape[1:]) == dy.shape
    yr.backward(torch.from_numpy(dy)[None])
    dw, db = _wgrad_walk(dy, x, k, d, s)
    assert np.allclose(dw, wr.grad.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(db, dy.sum(1), rtol=0, atol=1e-12)


# ---- the C ABI ----
def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd = C.c_void_p(16), C.c_void_p(18)      # never dereferenced: every call below fails (or finishes) before a launch

    def down(x=dummy, w=dummy, bias=dummy, y=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3):
        return lib.adk_enc_down(x, w, bias, y, n, cin, t, cout, k, s, None)

    def down_grad(dy=dummy, w=dummy, dx=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3):
        return lib.adk_enc_down_grad(dy, w, dx, n, cin, t, cout, k, s, None)

    def wgrad(dy=dummy, x=dummy, dw=dummy, db=dummy, ws=dummy, n=2, cin=8, t=100, cout=16, k=7, d=3, s=1, act=1, alpha=1.0):
        return lib.adk_conv_wgrad(dy, x, dw, db, ws, n, cin, t, cout, k, d, s, act, C.c_float(alpha), None)

    def plan(n=2, cin=8, t=100, cout=16, k=7, d=3, s=1):
        return lib.adk_conv_wgrad_plan(n, cin, t, cout, k, d, s, None, None)

    for name, fn, needed, optional in (("adk_enc_down", down, ("x", "w", "y"), ("bias",)),
                                       ("adk_enc_down_grad", down_grad, ("dy", "w", "dx"), ())):
        for kw in ({"n": -1}, {"cin": 0}, {"t": 0}, {"cout": 0}, {"k": 0}, {"s": 0}, {"k": 0, "s": 0}, {"t": -5}):
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        for kw in ({"k": 7}, {"k": 3}, {"k": 6, "s": 2}, {"k": 140000, "s": 70000}):
            assert fn(**kw) == ADK_ERR_ARG, (name, kw)
        assert fn(k=7) == ADK_ERR_ARG and b"2 * stride" in lib.adk_last_error()
        for p in needed:
            assert fn(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), (name, p)
        for p in needed + optional:
            assert fn(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), (name, p)
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(n=1 << 20, t=1 << 20) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(cin=1 << 28) == ADK_ERR_ARG and fn(cout=1 << 28) == ADK_ERR_ARG, name
        assert fn(**{"n": 0, **{p: None for p in needed + optional}}) == 0, name                 # nothing to do: no launch

    for name, fn in (("adk_conv_wgrad", wgrad), ("adk_conv_wgrad_plan", plan)):
        for kw in ({"n": -1}, {"cin": 0}, {"t": 0}, {"cout": 0}, {"k": 0}, {"d": 0}, {"s": 0}, {"s": -1}):
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(n=1 << 16, t=1 << 16) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(cin=1 << 28) == ADK_ERR_ARG and fn(cout=1 << 28) == ADK_ERR_ARG and fn(d=1 << 29) == ADK_ERR_ARG, name
    for kw in ({"act": 2}, {"act": -1}, {"alpha": float("nan")}):
        assert wgrad(**kw) == ADK_ERR_ARG and b"adk_conv_wgrad" in lib.adk_last_error(), kw
    for p in ("dy", "x", "dw", "ws"):
        assert wgrad(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), p
    for p in ("dy", "x", "dw", "db", "ws"):
        assert wgrad(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), p
    assert plan() == 0 and plan(n=0) == 0


# ---- the slice rule ----
def _tiles(cin, cout, k):
    bm = 128 if cout >= 128 else 64 if cout >= 64 else 32
    return -(-cout // bm) * -(-(cin * k + 1) // 128)


@pytest.mark.parametrize("shape", [(16, 32, 48000, 32, 7, 1, 1), (16, 256, 800, 256, 7, 9, 1), (16, 256, 800, 512, 10, 1, 5),
                                   (16, 1, 48000, 32, 7, 1, 1), (1, 4, 1000, 8, 7, 1, 1), (3, 2, 1, 6, 7, 1, 1), (0, 2, 5, 6, 7, 1, 1),
                                   (2, 33, 37, 72, 7, 9, 1), (1, 512, 160, 64, 3, 1, 1)])
def test_wgrad_plan(lib, shape):
    n, cin, t, cout, k, d, s = shape
    ws, S = EG.wgrad_plan(*shape)
    assert (ws, S) == EG.wgrad_plan(*shape)                            # a function of the shape
    assert S >= 1 and ws == 4 * S * cout * (cin * k + 1)               # S partial [c_out][c_in k + 1] tiles
    steps = -(-n * EG.out_length(t, s) // 32)
    s0 = max(1, min(-(-512 // _tiles(cin, cout, k)), steps // 4))
    per = max(1, -(-steps // s0))
    assert S == max(1, -(-steps // per)) and S <= 512                  # the rule the header states
    assert (S - 1) * per < max(steps, 1)                               # no slice is empty


def test_wgrad_plan_splits_a_long_reduction(lib):
    best = max(EG.wgrad_plan(1, 4, r, 8, 7)[1] for r in (1, 100, 1000, 4096, 65536))
    assert best >= 3
    assert EG.wgrad_plan(1, 4, 65536, 8, 7)[1] >= 3 and EG.wgrad_plan(1, 4, 1000, 8, 7)[1] >= 3
    assert EG.wgrad_plan(1, 4, 16, 8, 7)[1] == 1


# ---- host side of TrainableEncoder ----
def test_construction_and_shape_errors_without_device():
    with pytest.raises(NotImplementedError, match="weight_g"):
        EG.TrainableEncoder(use_weight_norm=True)
    with pytest.raises(NotImplementedError, match="causal"):
        EG.TrainableEncoder(mode="noncausal")
    with pytest.raises(NotImplementedError, match="ELU"):
        EG.TrainableEncoder(nonlinear_activation="LeakyReLU")
    with pytest.raises(NotImplementedError, match="ActivateEncoder"):
        EG.TrainableEncoder(codec="activate_audiodec")
    with pytest.raises(NotImplementedError, match="conv1d projector"):
        EG.TrainableEncoder(projector="conv1d_bn")
    with pytest.raises(ValueError, match="same length"):
        EG.TrainableEncoder(enc_ratios=(2, 4, 8), enc_strides=(3, 4, 5, 5))
    with pytest.raises(TypeError, match="unexpected keyword"):
        EG.TrainableEncoder(channels=3)
    enc = EG.TrainableEncoder()
    assert enc.hop == 300 and enc.out_frames(301) == 2 and enc.out_frames(3300) == 11 and enc.out_frames(1) == 1
    assert all(p.device.type == "cpu" and p.dtype == torch.float32 and p.requires_grad for p in enc.parameters())
    for bad in (torch.zeros(1, 2, 30), torch.zeros(1, 30), torch.zeros(1, 1, 30, 1), torch.zeros(0, 1, 30), torch.zeros(1, 1, 0)):
        with pytest.raises(ValueError, match="expected a|empty input"):
            enc(bad)
    # what a differentiable pass keeps: the input of every conv
    c = [32, 64, 128, 256]
    t = [300, 100, 25, 5]
    want = 300 + sum(7 * ci * ti for ci, ti in zip(c, t)) + 512
    assert enc.saved_floats(1, 300) == want


def test_parameter_names_and_state_dict(fixture):
    enc_tag, pe = MEG.generator_params("vctk_sym")
    enc = EG.TrainableEncoder(**pe)
    names = [k for k, _ in enc.named_parameters()]
    for case in MEG.CASES:
        assert names == [str(k) for k in fixture[f"{case}_names"]]
    assert names[0] == "encoder.conv.conv.weight" and names[-1] == "projector.project.conv.weight"
    assert "encoder.conv_blocks.2.res_units.1.conv2.weight" in names and "encoder.conv_blocks.3.conv.conv.bias" in names
    assert list(enc.state_dict()) == names
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    assert any(k.startswith("decoder.") for k in sd) and any(k.endswith(".pad_buffer") for k in sd)
    enc.load_state_dict(sd)                                            # the generator's dict: the rest is ignored
    for k, p in enc.named_parameters():
        assert torch.equal(p.detach(), sd[k]) and p.data_ptr() != sd[k].data_ptr()
    with pytest.raises(RuntimeError, match="Missing key"):
        EG.TrainableEncoder(**pe).load_state_dict({k: v for k, v in sd.items() if k != "projector.project.conv.weight"})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        EG.TrainableEncoder(**pe).load_state_dict(dict(sd, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch"):
        EG.TrainableEncoder(**pe).load_state_dict(dict(sd, **{"encoder.conv.conv.weight": torch.zeros(32, 2, 7)}))
    # the merged dict loads back into the streaming generator
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    with torch.no_grad():
        enc.get_parameter("encoder.conv.conv.weight").mul_(2.0)
    gen = AutoEncoderStreamGenerator(**pe)
    gen.load_state_dict({**sd, **enc.state_dict()})
    assert torch.equal(gen._sd["encoder.conv.conv.weight"], 2.0 * sd["encoder.conv.conv.weight"])
    assert torch.equal(gen._sd["decoder.conv1.conv.weight"], sd["decoder.conv1.conv.weight"])
    stereo = EG.TrainableEncoder(**MEG.generator_params("test_stereo_sym")[1])
    assert stereo.input_channels == 2 and stereo.get_parameter("encoder.conv.conv.weight").shape == (32, 2, 7)


def test_packs_follow_the_parameter_version():
    layer = EG._Layer(EG.arch.ConvSpec("op", "conv", 3, 4, 6, 3, 1, 1, True, False), EG.ACT_NONE, 1.0)
    w = torch.nn.Parameter(torch.randn(4, 3, 6))
    wf, wg = layer.packs(w)
    assert layer.packs(w)[0] is wf and layer.packs(w)[1] is wg         # not rebuilt on every call
    assert torch.equal(wf, DG.pack_conv(w.detach())) and torch.equal(wg, EG.pack_down_grad(w.detach(), 3))
    assert not wf.requires_grad and not wg.requires_grad
    with torch.no_grad():
        w.add_(1.0)                                                    # what an optimizer step does
    wf2, wg2 = layer.packs(w)
    assert wf2 is not wf and torch.equal(wf2, DG.pack_conv(w.detach())) and torch.equal(wg2, EG.pack_down_grad(w.detach(), 3))


# ---- the fixture ----
@pytest.mark.parametrize("name", list(MEG.CASES))
def test_fixture_is_consistent(fixture, name):
    model, shape = MEG.CASES[name]
    enc = EG.TrainableEncoder(**MEG.generator_params(model)[1])
    assert int(fixture[f"{name}_seed"]) == MEG.case_seed(name)
    x = MEG.case_input(name)
    assert x.shape == shape and x.dtype == np.float32
    z64, gx64 = fixture[f"{name}_z64"], fixture[f"{name}_gx64"]
    assert z64.dtype == np.float64 and z64.shape == (shape[0], 64, enc.out_frames(shape[2])) and gx64.shape == shape
    names = [str(k) for k in fixture[f"{name}_names"]]
    mx, er = fixture[f"{name}_max"], fixture[f"{name}_E_ref"]
    assert len(mx) == len(er) == len(names) + 2
    assert mx[0] == np.abs(z64).max() and mx[1] == np.abs(gx64).max()
    for i, (k, p) in enumerate(enc.named_parameters()):
        g = fixture[f"{name}_g{i}"]
        assert g.dtype == np.float64 and g.shape == MEG.sample(np.empty(p.numel())).shape and np.isfinite(g).all()
        assert 0 < np.abs(g).max() <= mx[i + 2]
    for e, m in zip(er, mx):
        assert 0 < e and 4 * e + 1e-6 * m <= MEG.CAP * m                # the cap: the bound cannot hide a dropped tap
    if name == "ragged":
        t, lens = shape[2], []
        for s in (3, 4, 5, 5):
            t = EG.out_length(t, s)
            lens.append(t)
        assert lens == [101, 26, 6, 2] and all(a % s for a, s in zip([301, 101, 26, 6], (3, 4, 5, 5)))
