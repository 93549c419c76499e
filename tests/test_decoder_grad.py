"""CPU: the frozen decoder's backward to its input -- host side, and what tests/golden/decoder_grad.npz means.

  * the four weight packings against NumPy restatements that walk the packed weights the way the kernels do, checked against
    torch's f64 conv / transposed conv and their autograd;
  * adk_dec_conv, adk_dec_conv_grad, adk_dec_convtr, adk_dec_convtr_grad and adk_rvq_st_grad are in the header and bound, the ABI
    is 14, and their argument checks run on the host before any HIP call;
  * FrozenDecoder's construction, loading and shape errors are raised before any device is touched;
  * the fixture: the stored caps hold, the gradients are finite and non-zero, and the quantizer gradient is the closed form
    dz = up + w[0] 2 (z - q0) / (rows dim) computed in NumPy from the stored z and the synthetic codebook.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_decoder_grad_golden as MDG
import make_forward_golden as MFG
from audiodec_amd import decoder_grad as DG
from audiodec_amd import synth

ADK_ERR_ARG = -1
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = (64, 1, 32, (16, 8, 4, 2), (5, 5, 4, 3))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "decoder_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def forward_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "forward.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


# ---- packings ----
@pytest.mark.parametrize("cin,cout,k,d,T", [(3, 5, 7, 1, 9), (4, 2, 7, 3, 20), (5, 3, 7, 9, 37), (6, 6, 1, 1, 4)])
def test_conv_packings(cin, cout, k, d, T):
    rng = np.random.default_rng(cin + cout + k + d)
    w = rng.standard_normal((cout, cin, k))
    x, dy = rng.standard_normal((cin, T)), rng.standard_normal((cout, T))
    pf, pg = DG.pack_conv(torch.from_numpy(w)).numpy(), DG.pack_conv_grad(torch.from_numpy(w)).numpy()
    assert pf.shape == (cin * k, cout) and pg.shape == (cout * k, cin)
    y, dx = np.zeros((cout, T)), np.zeros((cin, T))
    for u in range(T):
        for kk in range(cin * k):                              # forward GEMM: kk = ci k + j reads x[ci][u - (k-1-j) d]
            ci, j = divmod(kk, k)
            t = u - (k - 1 - j) * d
            if t >= 0:
                y[:, u] += pf[kk] * x[ci, t]
        for kk in range(cout * k):                             # backward GEMM: kk = co k + j reads dy[co][u + (k-1-j) d]
            co, j = divmod(kk, k)
            t = u + (k - 1 - j) * d
            if t < T:
                dx[:, u] += pg[kk] * dy[co, t]
    xr = torch.from_numpy(x)[None].requires_grad_(True)
    yr = F.conv1d(F.pad(xr, ((k - 1) * d, 0)), torch.from_numpy(w), dilation=d)
    yr.backward(torch.from_numpy(dy)[None])
    assert np.allclose(y, yr.detach().numpy()[0], rtol=0, atol=1e-12)
    assert np.allclose(dx, xr.grad.numpy()[0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("cin,cout,s,T", [(3, 4, 3, 1), (4, 2, 4, 2), (5, 3, 5, 7)])
def test_convtr_packings(cin, cout, s, T):
    rng = np.random.default_rng(cin + cout + s + T)
    w = rng.standard_normal((cin, cout, 2 * s))
    x, dy = rng.standard_normal((cin, T)), rng.standard_normal((cout, T * s))
    pf, pg = DG.pack_convtr(torch.from_numpy(w), s).numpy(), DG.pack_convtr_grad(torch.from_numpy(w), s).numpy()
    assert pf.shape == (s, 2 * cin, cout) and pg.shape == (cout * 2 * s, cin)
    y, dx = np.zeros((cout, T * s)), np.zeros((cin, T))
    for i in range(T):
        for r in range(s):                                     # forward: one GEMM per phase, kk = 2 ci + tap
            for kk in range(2 * cin):
                ci, tap = divmod(kk, 2)
                y[:, i * s + r] += pf[r, kk] * x[ci, max(i - 1, 0) if tap else i]
        for kk in range(cout * 2 * s):                         # backward: kk = co 2s + q
            co, q = divmod(kk, 2 * s)
            g = dy[co, i * s + q] if i * s + q < T * s else 0.0
            if i == 0 and q >= s:
                g += dy[co, q - s]
            dx[:, i] += pg[kk] * g
    xr = torch.from_numpy(x)[None].requires_grad_(True)
    yr = F.conv_transpose1d(F.pad(xr, (1, 0), mode="replicate"), torch.from_numpy(w), stride=s)[:, :, s:-s]
    yr.backward(torch.from_numpy(dy)[None])
    assert np.allclose(y, yr.detach().numpy()[0], rtol=0, atol=1e-12)
    assert np.allclose(dx, xr.grad.numpy()[0], rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="2 \\* stride"):
        DG.pack_convtr(torch.from_numpy(w), s + 1)
    with pytest.raises(ValueError, match="2 \\* stride"):
        DG.pack_convtr_grad(torch.from_numpy(w), s + 1)


# ---- the C ABI ----
def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name in ("adk_dec_conv", "adk_dec_conv_grad", "adk_dec_convtr", "adk_dec_convtr_grad", "adk_rvq_st_grad"):
        assert f"int {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd = C.c_void_p(16), C.c_void_p(18)      # never dereferenced: every call below fails (or finishes) before a launch

    def conv(x=dummy, w=dummy, bias=dummy, res=dummy, y=dummy, n=2, cin=8, t=100, cout=16, k=7, d=3, act=1, alpha=1.0, impl=2):
        return lib.adk_dec_conv(x, w, bias, res, y, n, cin, t, cout, k, d, act, C.c_float(alpha), impl, None)

    def conv_grad(dy=dummy, x=dummy, w=dummy, dres=dummy, dx=dummy, n=2, cin=8, t=100, cout=16, k=7, d=3, act=1, alpha=1.0):
        return lib.adk_dec_conv_grad(dy, x, w, dres, dx, n, cin, t, cout, k, d, act, C.c_float(alpha), None)

    def convtr(x=dummy, w=dummy, bias=dummy, y=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=1, alpha=1.0):
        return lib.adk_dec_convtr(x, w, bias, y, n, cin, t, cout, k, s, act, C.c_float(alpha), None)

    def convtr_grad(dy=dummy, x=dummy, w=dummy, dx=dummy, n=2, cin=8, t=100, cout=16, k=6, s=3, act=1, alpha=1.0):
        return lib.adk_dec_convtr_grad(dy, x, w, dx, n, cin, t, cout, k, s, act, C.c_float(alpha), None)

    def st(dzq=dummy, up=dummy, z=dummy, cb=dummy, idx=dummy, dz=dummy, n=2, dim=64, t=10, size=1024):
        return lib.adk_rvq_st_grad(dzq, up, z, cb, idx, dz, n, dim, t, size, None)

    calls = {"adk_dec_conv": (conv, "d", ("x", "w", "y"), ("bias", "res")),
             "adk_dec_conv_grad": (conv_grad, "d", ("dy", "x", "w", "dx"), ("dres",)),
             "adk_dec_convtr": (convtr, "s", ("x", "w", "y"), ("bias",)),
             "adk_dec_convtr_grad": (convtr_grad, "s", ("dy", "x", "w", "dx"), ())}
    for name, (fn, step, needed, optional) in calls.items():
        for kw in ({"n": -1}, {"cin": 0}, {"t": 0}, {"cout": 0}, {"k": 0}, {step: 0}, {"act": 2}, {"act": -1}, {"alpha": float("nan")}):
            assert fn(**kw) == ADK_ERR_ARG and name.encode() in lib.adk_last_error(), (name, kw)
        for p in needed:
            assert fn(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), (name, p)
        for p in needed + optional:
            assert fn(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), (name, p)
        assert fn(t=1 << 30) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name      # extents that overflow
        assert fn(n=1 << 20, t=1 << 20) == ADK_ERR_ARG and b"too large" in lib.adk_last_error(), name
        assert fn(cin=1 << 28) == ADK_ERR_ARG and fn(cout=1 << 28) == ADK_ERR_ARG, name
        assert fn(**{"n": 0, **{p: None for p in needed + optional}}) == 0, name                 # nothing to do: no launch
    assert conv(impl=0) == ADK_ERR_ARG and conv(impl=3) == ADK_ERR_ARG and b"impl" in lib.adk_last_error()
    assert conv(d=1 << 29) == ADK_ERR_ARG and conv_grad(d=1 << 29) == ADK_ERR_ARG
    for fn in (convtr, convtr_grad):
        assert fn(k=7) == ADK_ERR_ARG and b"2 * stride" in lib.adk_last_error()
        assert fn(k=140000, s=70000) == ADK_ERR_ARG
    # without an input activation the backward does not read x
    assert conv_grad(act=0, x=None, n=0) == 0
    for kw in ({"n": -1}, {"dim": 0}, {"t": 0}, {"size": 0}):
        assert st(**kw) == ADK_ERR_ARG and b"adk_rvq_st_grad" in lib.adk_last_error(), kw
    for p in ("z", "cb", "idx", "dz"):
        assert st(**{p: None}) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), p
    for p in ("dzq", "up", "z", "cb", "dz", "idx"):
        assert st(**{p: odd}) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), p
    assert st(idx=C.c_void_p(20)) == ADK_ERR_ARG and b"8-byte" in lib.adk_last_error()
    assert st(n=1 << 16, t=1 << 16) == ADK_ERR_ARG and b"too large" in lib.adk_last_error()
    assert st(n=0, dzq=None, up=None, z=None, cb=None, idx=None, dz=None) == 0


# ---- host side of FrozenDecoder ----
def test_construction_and_shape_errors_without_device():
    with pytest.raises(NotImplementedError, match="causal"):
        DG.FrozenDecoder(*ARGS, mode="noncausal")
    with pytest.raises(NotImplementedError, match="ELU"):
        DG.FrozenDecoder(*ARGS, nonlinear_activation="LeakyReLU")
    with pytest.raises(NotImplementedError, match="ActivateDecoder"):
        DG.FrozenDecoder(*ARGS, codec="activate_audiodec")
    with pytest.raises(ValueError, match="same length"):
        DG.FrozenDecoder(64, 1, 32, (16, 8, 4, 2), (5, 5, 4))
    dec = DG.FrozenDecoder(*ARGS)
    assert dec.device is None and dec.hop == 300 and dec.weights() == []
    with pytest.raises(RuntimeError, match="no weights loaded"):
        dec(torch.zeros(1, 64, 3))
    enc_tag, _ = MDG.generator_params("vctk_sym")
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    dec.load_state_dict(sd)                                            # the generator's keys, others ignored
    own = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
    dec2 = DG.FrozenDecoder(*ARGS).load_state_dict(own)                # the decoder's own keys
    for (s1, w1, b1), (s2, w2, b2) in zip(dec._host, dec2._host):
        assert s1.name == s2.name and torch.equal(w1, w2) and (b1 is None) == (b2 is None) and (b1 is None or torch.equal(b1, b2))
    assert [s.name for s, _, _ in dec._host][:3] == ["decoder.conv1", "decoder.conv_blocks.0.conv", "decoder.conv_blocks.0.res_units.0.conv1"]
    for bad in (torch.zeros(1, 63, 3), torch.zeros(64, 3), torch.zeros(1, 64, 3, 1)):
        with pytest.raises(ValueError, match="expected a"):
            dec(bad)
    incomplete = {k: v for k, v in own.items() if k != "conv2.conv.weight"}
    with pytest.raises(RuntimeError, match="missing keys"):
        DG.FrozenDecoder(*ARGS).load_state_dict(incomplete)
    wrong = dict(own, **{"conv2.conv.weight": torch.zeros(2, 32, 7)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        DG.FrozenDecoder(*ARGS).load_state_dict(wrong)
    # what a differentiable pass keeps: two tensors per residual unit
    assert dec.saved_floats(1, 1) == 2 * 3 * (256 * 5 + 128 * 25 + 64 * 100 + 32 * 300)


def test_weight_norm_is_folded_as_the_generators_fold_it():
    rng = np.random.default_rng(3)
    enc_tag, _ = MDG.generator_params("vctk_sym")
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    wn = {}
    for k, v in sd.items():
        if k.startswith("decoder.") and k.endswith(".weight"):
            g = torch.from_numpy(rng.uniform(0.5, 2.0, size=(v.shape[0], 1, 1)).astype(np.float32))
            wn[k[:-len("weight")] + "weight_g"], wn[k[:-len("weight")] + "weight_v"] = g, v
        elif k.startswith("decoder."):
            wn[k] = v
    dec = DG.FrozenDecoder(*ARGS, use_weight_norm=True).load_state_dict(wn)
    for s, w, _ in dec._host:
        assert torch.equal(w, torch._weight_norm(wn[s.wkey("weight_v")], wn[s.wkey("weight_g")], 0))


# ---- the fixture ----
@pytest.mark.parametrize("name", list(MDG.CASES))
def test_fixture_is_consistent(fixture, forward_fixture, name):
    model, fcase, sl = MDG.CASES[name]
    assert tuple(fixture[f"{name}_slice"]) == sl and int(fixture[f"{name}_seed"]) == MDG.case_seed(name)
    zq = MDG.case_slice(forward_fixture[f"{fcase}_zq"], sl)
    y64, g64 = fixture[f"{name}_y64"], fixture[f"{name}_grad64"]
    assert y64.dtype == np.float64 and g64.dtype == np.float64 and g64.shape == zq.shape
    assert y64.shape[0] == zq.shape[0] and y64.shape[2] == zq.shape[2] * 300
    for k, ref in (("y", y64), ("g", g64)):
        e, m = float(fixture[f"{name}_E_ref_{k}"]), float(fixture[f"{name}_max_{k}"])
        assert m == float(np.abs(ref).max()) and 0 < e
        assert 4 * e + 1e-6 * m <= 1e-5 * m, (name, k, e, m)          # the cap: the bound cannot hide a wrong tap
    assert np.isfinite(y64).all() and np.isfinite(g64).all() and np.abs(g64).max() > 0 and np.count_nonzero(g64) == g64.size


@pytest.mark.parametrize("name", list(MDG.CASES))
def test_fixture_quantizer_gradient_is_the_closed_form(fixture, forward_fixture, name):
    model, fcase, sl = MDG.CASES[name]
    enc_tag, pe = MDG.generator_params(model)
    embed0 = synth.synth_state_dict(enc_tag, MFG.SEED)["quantizer.codebook.layers.0.embed"].numpy().astype(np.float64)   # (dim, size)
    z = MDG.case_slice(forward_fixture[f"{fcase}_z"], sl).astype(np.float64)
    B, D, T = z.shape
    idx0 = fixture[f"{name}_q_idx0"].astype(np.int64).reshape(B, T)
    rows = z.transpose(0, 2, 1).reshape(-1, D)
    dist = (rows ** 2).sum(1, keepdims=True) - 2 * rows @ embed0 + (embed0 ** 2).sum(0, keepdims=True)
    assert np.array_equal(dist.argmin(1).reshape(B, T), idx0)          # the stored codes are stage 0's nearest codes
    q0 = embed0.T[idx0].transpose(0, 2, 1)                             # (B, D, T)
    up = MDG.upstream(int(fixture[f"{name}_seed"]) + 1, z.shape).astype(np.float64)
    want = up + 1.0 * 2.0 * (z - q0) / (B * T * D)                     # w[0] = 1; stages >= 1 pass nothing
    got = fixture[f"{name}_q_grad"]
    assert got.dtype == np.float32 and got.shape == z.shape
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
