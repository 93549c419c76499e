"""GPU: the frozen symmetric decoder's forward and backward to its input, and the quantizer's straight-through step
(adk_dec_conv, adk_dec_convtr, their _grad calls, adk_rvq_st_grad; audiodec_amd/decoder_grad.py).

  A. op level, exact: small integer weights, inputs and upstreams make every f32 sum exact, so forward and gradient must
     torch.equal the f64 torch restatement cast to f32 -- with no activation, and with ELU on strictly positive inputs (where ELU
     is the identity), over the shapes that can break the indexing;
  B. ELU's negative side: the same ops on real-valued inputs against f64, bound 4 E + 1e-6 max, E the f32 torch CPU error of the
     same op computed here;
  C. whole decoder: every case of decoder_grad.npz within 4 E_ref + 1e-6 max of the f64 reference (E_ref the reference's own f32
     error), output and gradient; the full zq of forward.npz's cases within the waveform bound of the stored y;
  D. quantize_st: values bitwise those of quantizer_forward(return_stats=True), z.grad against the reference's;
  E. behaviour: bitwise reproducibility, no graph without need, constant weights, the second backward, the chain through the
     mel loss, the construction errors.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_decoder_grad_golden as MDG
import make_forward_golden as MFG
from audiodec_amd import arch, configs, synth

pytestmark = pytest.mark.gpu
WAVE_TOL = 1e-4


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "decoder_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def forward_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "forward.npz"), allow_pickle=False)


def _layer(gpu, kind, cin, cout, k, stride, dil, w, b, act, alpha=1.0):
    from audiodec_amd import decoder_grad as DG
    spec = arch.ConvSpec("op", kind, cin, cout, k, stride, dil, 1, b is not None, False)
    return DG._Layer(spec, w, b, act, alpha, gpu)


def _conv_ref(x, w, b, res, k, d, act, alpha=1.0):
    """CausalConv1d.forward on a(x), plus the skip: the formula of the reference's layers in torch ops (any dtype)."""
    h = F.elu(x, alpha) if act else x
    y = F.conv1d(F.pad(h, ((k - 1) * d, 0)), w, b, dilation=d)
    return y + res if res is not None else y


def _convtr_ref(x, w, b, s, act, alpha=1.0):
    """CausalConvTranspose1d.forward on a(x) (layers/conv_layer.py:189-192)."""
    h = F.elu(x, alpha) if act else x
    return F.conv_transpose1d(F.pad(h, (1, 0), mode="replicate"), w, b, stride=s)[:, :, s:-s]


# ---- A. op level, exact ----
# (n_items, c_in, c_out, kernel, dilation, T, residual, bias)
CONV_CASES = {
    "cin32_n127": (1, 32, 6, 7, 1, 127, False, True),             # the 32-row tile, one column short of a tile; K = 42
    "cin33_n129_d3": (1, 33, 4, 7, 3, 129, False, False),         # M edge; a second column tile of one column; K = 28
    "cin64_d9_t37": (2, 64, 5, 7, 9, 37, False, True),            # the 64-row tile; T < 54: every column has causal zeros; K = 35
    "cin128_n1": (1, 128, 8, 7, 1, 1, False, True),               # the 128-row tile; a single column
    "cin160_items_d3": (3, 160, 40, 7, 3, 40, False, True),       # 128-row tile with an M edge; three items inside column tile 0
    "cin32_d9": (1, 32, 12, 7, 9, 130, False, False),
    "k1_res_cin32": (2, 32, 32, 1, 1, 50, True, False),           # the residual unit's 1x1 with its skip
    "k1_res_cin64_n129": (1, 64, 64, 1, 1, 129, True, True),
    "k7_res_cin33": (3, 33, 33, 7, 3, 43, True, False),           # skip on a dilated conv: the backward's dres at an M edge
    "direct_cout1": (2, 32, 1, 7, 1, 129, False, False),          # conv2, mono: the direct kernel; backward K = 7
    "direct_cout2": (1, 32, 2, 7, 1, 127, False, True),           # conv2, stereo; backward K = 14
    "fwd_cout72": (1, 8, 72, 7, 1, 130, False, True),             # the forward's 64-row tile with an M edge
    "fwd_cout136_k1": (2, 4, 136, 1, 1, 33, False, True),         # the forward's 128-row tile with an M edge
}


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_exact(gpu, name, elu):
    from audiodec_amd import decoder_grad as DG
    n, cin, cout, k, d, T, has_res, has_bias = CONV_CASES[name]
    rng = np.random.default_rng(n + cin + cout + k + d + T)
    w = _ints(rng, -3, 3, (cout, cin, k))
    b = _ints(rng, -2, 2, (cout,)) if has_bias else None
    x = _ints(rng, 1, 4, (n, cin, T)) if elu else _ints(rng, -4, 4, (n, cin, T))
    res = _ints(rng, -5, 5, (n, cout, T)) if has_res else None
    dy = _ints(rng, -3, 3, (n, cout, T))
    dres = _ints(rng, -5, 5, (n, cin, T)) if has_res else None
    layer = _layer(gpu, "conv" if k > 1 else "conv1x1", cin, cout, k, 1, d, w, b, DG.ACT_ELU if elu else DG.ACT_NONE)
    assert layer.impl == (DG.IMPL_DIRECT if cout <= 2 else DG.IMPL_GEMM)
    xr = x.double().requires_grad_(True)
    yr = _conv_ref(xr, w.double(), b.double() if has_bias else None, res.double() if has_res else None, k, d, elu)
    yr.backward(dy.double())
    want_dx = xr.grad + dres.double() if has_res else xr.grad
    xg = x.to(gpu)
    y = layer(xg, res=res.to(gpu) if has_res else None)
    assert torch.equal(y.cpu(), yr.detach().float()), f"{name}: forward max diff {float((y.cpu() - yr.detach().float()).abs().max())}"
    dx = layer.grad(dy.to(gpu), xg if elu else None, tuple(x.shape), dres=dres.to(gpu) if has_res else None)
    assert dx.shape == x.shape and dx.dtype == torch.float32
    assert torch.equal(dx.cpu(), want_dx.float()), f"{name}: grad max diff {float((dx.cpu() - want_dx.float()).abs().max())}"
    assert float(xr.grad.abs().max()) > 0


@pytest.mark.parametrize("chans", [(64, 32), (33, 5)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("s", [3, 4, 5])
def test_convtr_exact(gpu, s, T, n, chans):
    from audiodec_amd import decoder_grad as DG
    cin, cout = chans
    rng = np.random.default_rng(1000 * s + 100 * T + 10 * n + cin)
    w = _ints(rng, -3, 3, (cin, cout, 2 * s))
    b = _ints(rng, -2, 2, (cout,))
    dy = _ints(rng, -3, 3, (n, cout, T * s))
    for elu in (False, True):
        x = _ints(rng, 1, 4, (n, cin, T)) if elu else _ints(rng, -4, 4, (n, cin, T))
        layer = _layer(gpu, "convT", cin, cout, 2 * s, s, 1, w, b, DG.ACT_ELU if elu else DG.ACT_NONE)
        xr = x.double().requires_grad_(True)
        yr = _convtr_ref(xr, w.double(), b.double(), s, elu)
        assert tuple(yr.shape) == (n, cout, T * s)
        yr.backward(dy.double())
        xg = x.to(gpu).requires_grad_(True)
        y = DG._ConvFn.apply(xg, layer)
        assert y.requires_grad and torch.equal(y.detach().cpu(), yr.detach().float()), f"forward, elu={elu}"
        y.backward(dy.to(gpu))
        assert torch.equal(xg.grad.cpu(), xr.grad.float()), f"grad, elu={elu}: max diff {float((xg.grad.cpu() - xr.grad.float()).abs().max())}"
        assert float(xr.grad.abs().max()) > 0


# ---- B. ELU's negative side ----
def _real(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _bounded(got, ref64, ref32, what):
    """max|got - ref64| <= 4 E + 1e-6 max|ref64|, E = max|ref32 - ref64| (torch's f32 on the CPU)."""
    e, m = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err = float((got.cpu().double() - ref64).abs().max())
    bound = 4 * e + 1e-6 * m
    print(f"{what}: err {err:.3e} E {e:.3e} max {m:.3f} err/bound {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


ELU_CONV_CASES = ["cin33_n129_d3", "cin64_d9_t37", "cin160_items_d3", "k1_res_cin64_n129", "k7_res_cin33", "direct_cout2"]


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", ELU_CONV_CASES)
def test_conv_elu_negative_side(gpu, name, alpha):
    from audiodec_amd import decoder_grad as DG
    n, cin, cout, k, d, T, has_res, has_bias = CONV_CASES[name]
    rng = np.random.default_rng(7 + n + cin + cout + k + d + T)
    w = _real(rng, (cout, cin, k), 1.0 / np.sqrt(cin * k))
    b = _real(rng, (cout,)) if has_bias else None
    x = _real(rng, (n, cin, T), 1.5)
    assert float((x < 0).float().mean()) > 0.3
    res = _real(rng, (n, cout, T)) if has_res else None
    dy = _real(rng, (n, cout, T))
    dres = _real(rng, (n, cin, T)) if has_res else None
    out = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).requires_grad_(True)
        yr = _conv_ref(xr, w.to(dt), b.to(dt) if has_bias else None, res.to(dt) if has_res else None, k, d, True, alpha)
        yr.backward(dy.to(dt))
        out[dt] = (yr.detach(), xr.grad + dres.to(dt) if has_res else xr.grad)
    layer = _layer(gpu, "conv" if k > 1 else "conv1x1", cin, cout, k, 1, d, w, b, DG.ACT_ELU, alpha)
    xg = x.to(gpu)
    y = layer(xg, res=res.to(gpu) if has_res else None)
    dx = layer.grad(dy.to(gpu), xg, tuple(x.shape), dres=dres.to(gpu) if has_res else None)
    _bounded(y, out[torch.float64][0], out[torch.float32][0], f"{name} alpha {alpha} forward")
    _bounded(dx, out[torch.float64][1], out[torch.float32][1], f"{name} alpha {alpha} grad")


@pytest.mark.parametrize("s,T,n,cin,cout", [(3, 7, 3, 64, 32), (5, 1, 1, 33, 5), (4, 2, 3, 33, 5), (5, 40, 2, 128, 64)])
def test_convtr_elu_negative_side(gpu, s, T, n, cin, cout):
    from audiodec_amd import decoder_grad as DG
    rng = np.random.default_rng(s + T + n + cin)
    w = _real(rng, (cin, cout, 2 * s), 1.0 / np.sqrt(2 * cin))
    b = _real(rng, (cout,))
    x = _real(rng, (n, cin, T), 1.5)
    dy = _real(rng, (n, cout, T * s))
    out = {}
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).requires_grad_(True)
        yr = _convtr_ref(xr, w.to(dt), b.to(dt), s, True)
        yr.backward(dy.to(dt))
        out[dt] = (yr.detach(), xr.grad)
    layer = _layer(gpu, "convT", cin, cout, 2 * s, s, 1, w, b, DG.ACT_ELU)
    xg = x.to(gpu)
    y = layer(xg)
    dx = layer.grad(dy.to(gpu), xg, tuple(x.shape))
    _bounded(y, out[torch.float64][0], out[torch.float32][0], f"convtr s{s} T{T} forward")
    _bounded(dx, out[torch.float64][1], out[torch.float32][1], f"convtr s{s} T{T} grad")


# ---- C. whole decoder ----
def _decoder(gpu, model):
    from audiodec_amd import decoder_grad as DG
    enc_tag, pe = MDG.generator_params(model)
    dec = DG.FrozenDecoder(pe["code_dim"], pe["output_channels"], pe["decode_channels"], pe["dec_ratios"], pe["dec_strides"],
                           device=gpu)
    return dec.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))


def _generator(gpu, model):
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    enc_tag, pe = MDG.generator_params(model)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return g.eval().to(gpu)


@pytest.mark.parametrize("name", list(MDG.CASES))
def test_decoder_against_reference(gpu, fixture, forward_fixture, name):
    model, fcase, sl = MDG.CASES[name]
    assert tuple(fixture[f"{name}_slice"]) == sl
    dec = _decoder(gpu, model)
    zq = torch.from_numpy(MDG.case_slice(forward_fixture[f"{fcase}_zq"], sl)).to(gpu).requires_grad_(True)
    y = dec(zq)
    y64, g64 = fixture[f"{name}_y64"], fixture[f"{name}_grad64"]
    assert tuple(y.shape) == y64.shape and y.requires_grad
    up = torch.from_numpy(MDG.upstream(int(fixture[f"{name}_seed"]), y64.shape)).to(gpu)
    y.backward(up)
    for k, got, ref in (("y", y.detach(), y64), ("g", zq.grad, g64)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        bound = 4 * float(fixture[f"{name}_E_ref_{k}"]) + 1e-6 * float(np.abs(ref).max())
        print(f"decoder {name} {k}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound, f"{name} {k}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(MFG.FORWARD))
def test_decoder_forward_matches_stored_waveform(gpu, forward_fixture, name):
    dec = _decoder(gpu, MFG.FORWARD[name][0])
    with torch.no_grad():
        y = dec(torch.from_numpy(forward_fixture[f"{name}_zq"]).to(gpu))
    ref = forward_fixture[f"{name}_y"]
    assert tuple(y.shape) == ref.shape
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"forward {name}: max|dy| {err:.3e} ratio {err / WAVE_TOL:.3f}")
    assert err <= WAVE_TOL


# ---- D. quantizer ----
@pytest.mark.parametrize("name", list(MDG.CASES))
def test_quantize_st(gpu, fixture, forward_fixture, name):
    from audiodec_amd import decoder_grad as DG
    model, fcase, sl = MDG.CASES[name]
    g = _generator(gpu, model)
    z_np = MDG.case_slice(forward_fixture[f"{fcase}_z"], sl)
    with torch.no_grad():
        ref = [t.clone() for t in g.quantizer_forward(torch.from_numpy(z_np).to(gpu), return_stats=True)]
        plain = DG.quantize_st(g, torch.from_numpy(z_np).to(gpu))
    z = torch.from_numpy(z_np).to(gpu).requires_grad_(True)
    zq, vq, ppl = DG.quantize_st(g, z)
    assert zq.requires_grad and vq.requires_grad and not ppl.requires_grad
    assert not any(t.requires_grad for t in plain)
    for a, b, c in zip((zq, vq, ppl), ref, plain):
        assert a.shape == b.shape and torch.equal(a.detach(), torch.as_tensor(b)) and torch.equal(c, torch.as_tensor(b))
    idx0 = g.quantize(torch.from_numpy(z_np).to(gpu)).reshape(g.n_q, -1)[0].cpu().numpy()
    assert np.array_equal(idx0.reshape(fixture[f"{name}_q_idx0"].shape), fixture[f"{name}_q_idx0"])
    up = torch.from_numpy(MDG.upstream(int(fixture[f"{name}_seed"]) + 1, tuple(zq.shape))).to(gpu)
    w = torch.arange(1, g.n_q + 1, dtype=torch.float32, device=gpu)
    ((zq * up).sum() + (vq * w).sum()).backward()
    want = fixture[f"{name}_q_grad"]
    err, m = float(np.abs(z.grad.cpu().numpy() - want).max()), float(np.abs(want).max())
    print(f"quantizer {name}: err {err:.3e} max {m:.3f} ratio {err / (1e-6 * m):.3f}")
    assert err <= 1e-6 * m


# ---- E. behaviour ----
def test_reproducible_graph_and_weights(gpu, forward_fixture):
    dec = _decoder(gpu, "vctk_sym")
    zq_np = MDG.case_slice(forward_fixture["b3_zq"], (0, 2, 0, 5))
    up = torch.from_numpy(MDG.upstream(5, (2, 1, 1500))).to(gpu)
    runs = []
    for _ in range(2):
        zq = torch.from_numpy(zq_np).to(gpu).requires_grad_(True)
        y = dec(zq)
        y.backward(up)
        runs.append((y.detach().clone(), zq.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # no graph under no_grad or for a constant input; the same output, bit for bit
    zq = torch.from_numpy(zq_np).to(gpu).requires_grad_(True)
    with torch.no_grad():
        y0 = dec(zq)
    y1 = dec(zq.detach())
    for y in (y0, y1):
        assert not y.requires_grad and y.grad_fn is None and torch.equal(y, runs[0][0])
    assert dec.weights() and not any(t.requires_grad for t in dec.weights())
    # once differentiable: the gradient is a constant to autograd, and an upstream that requires grad asks for the second derivative
    zz = torch.from_numpy(zq_np).to(gpu).requires_grad_(True)
    (g1,) = torch.autograd.grad(dec(zz), zz, up, create_graph=True)
    assert not g1.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        g1.sum().backward()
    w = torch.ones((), device=gpu, requires_grad=True)
    (g2,) = torch.autograd.grad(dec(zz), zz, up * w, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.sum().backward()


def test_from_generator_and_chain_through_mel(gpu, forward_fixture):
    """d mel(FrozenDecoder(quantize_st(z)[0]), y) / dz equals the decoder's backward applied to the mel loss's own y_hat gradient
    (the straight-through step passes it on unchanged): the Functions compose through torch.autograd."""
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import mel
    g = _generator(gpu, "vctk_sym")
    dec = DG.FrozenDecoder.from_generator(g)
    ref_dec = _decoder(gpu, "vctk_sym")
    z_np = MDG.case_slice(forward_fixture["b3_z"], (0, 2, 0, 11))
    target = torch.from_numpy(forward_fixture["b3_y"][:2, :, :3300]).to(gpu) * 0.9
    loss = mel.MultiMelSpectrogramLoss(fs=48000, device=gpu, differentiable=True)
    z = torch.from_numpy(z_np).to(gpu).requires_grad_(True)
    zq, _, _ = DG.quantize_st(g, z)
    y_hat = dec(zq)
    with torch.no_grad():
        assert torch.equal(y_hat.detach(), ref_dec(zq.detach()))
    loss(y_hat, target).backward()
    # the two steps by hand
    yh = y_hat.detach().clone().requires_grad_(True)
    loss(yh, target).backward()
    zq2 = zq.detach().clone().requires_grad_(True)
    ref_dec(zq2).backward(yh.grad)
    m = float(zq2.grad.abs().max())
    err = float((z.grad - zq2.grad).abs().max())
    print(f"chain: err {err:.3e} max {m:.3e}")
    assert m > 0 and err <= 1e-6 * m
    assert g._dec is None and g._enc is None                # no program was built or touched


def test_construction_errors():
    from audiodec_amd import decoder_grad as DG
    args = (64, 1, 32, (16, 8, 4, 2), (5, 5, 4, 3))
    with pytest.raises(NotImplementedError, match="causal"):
        DG.FrozenDecoder(*args, mode="noncausal")
    with pytest.raises(NotImplementedError, match="ELU"):
        DG.FrozenDecoder(*args, nonlinear_activation="LeakyReLU")
    with pytest.raises(NotImplementedError, match="ActivateDecoder"):
        DG.FrozenDecoder(*args, codec="activate_audiodec")
    _, enc_tag, _, _, _ = configs.alias("vctk_activate_sym")
    _, _, pe = configs.experiment(enc_tag)
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    gen = AutoEncoderStreamGenerator(**pe)
    gen.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    with pytest.raises(NotImplementedError, match="ActivateDecoder"):
        DG.FrozenDecoder.from_generator(gen)
