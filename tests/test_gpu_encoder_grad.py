"""GPU: the trainable encoder (adk_enc_down, adk_enc_down_grad, adk_conv_wgrad; audiodec_amd/encoder_grad.py).

  A. op level, exact: small integer weights, inputs and upstreams make every f32 sum exact, so forward, gradient to the input and
     weight / bias gradients must torch.equal the f64 torch restatement cast to f32 -- with no activation, and with ELU on strictly
     positive inputs (where ELU is the identity), over the shapes that can break the indexing;
  B. ELU's negative side and real values: the same ops against f64, bound 4 E + 1e-6 max, E the f32 torch CPU error of the same op
     computed here;
  C. whole encoder: every case of encoder_grad.npz within 4 E_ref + 1e-6 max of the f64 reference (E_ref the reference's own f32
     error): z, x.grad and every parameter's sampled gradient;
  D. the denoise step: the chain through quantize_st, FrozenDecoder and the mel loss fills every parameter's .grad, bitwise
     reproducibly, and the trained weights load back into the streaming generator;
  E. behaviour: no graph without need, frozen parameters launch no weight gradient, the second backward, construction errors.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_encoder_grad_golden as MEG
import make_forward_golden as MFG
from audiodec_amd import arch, configs, synth

pytestmark = pytest.mark.gpu
LATENT_TOL = 1e-4


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "encoder_grad.npz"), allow_pickle=False)


def _layer(cin, cout, k, stride, dil, act, alpha=1.0, bias=True):
    from audiodec_amd import encoder_grad as EG
    kind = "conv" if k > 1 else "conv1x1"
    return EG._Layer(arch.ConvSpec("op", kind, cin, cout, k, stride, dil, 1, bias, False), act, alpha)


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def _real(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _conv_ref(x, w, b, k, d, s, act, alpha=1.0):
    """CausalConv1d.forward on a(x): the formula of the reference's layer in torch ops (any dtype)."""
    h = F.elu(x, alpha) if act else x
    return F.conv1d(F.pad(h, ((k - 1) * d, 0)), w, b, stride=s, dilation=d)


def _ref_grads(x, w, b, dy, k, d, s, act, alpha, dt):
    """(y, dx, dw, db) of the conv in dtype dt on the CPU."""
    xr, wr, br = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
    y = _conv_ref(xr, wr, br, k, d, s, act, alpha)
    y.backward(dy.to(dt))
    return y.detach(), xr.grad, wr.grad, br.grad


def _bounded(got, ref64, ref32, what):
    """max|got - ref64| <= 4 E + 1e-6 max|ref64|, E = max|ref32 - ref64| (torch's f32 on the CPU)."""
    e, m = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err = float((got.cpu().double() - ref64).abs().max())
    bound = 4 * e + 1e-6 * m
    print(f"{what}: err {err:.3e} E {e:.3e} max {m:.3f} err/bound {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _wgrad(layer, dy, x, want_bias=True):
    """adk_conv_wgrad through the layer, on a workspace full of NaN (any contents)."""
    from audiodec_amd import encoder_grad as EG
    s = layer.spec
    ws = EG._Workspace()
    n_bytes, _ = EG.wgrad_plan(x.shape[0], s.cin, x.shape[2], s.cout, s.k, s.dilation, s.stride)
    ws.get(n_bytes, x.device).fill_(float("nan"))
    return layer.grad_weight(dy, x, ws, want_bias)


# ---- A. op level, exact ----
@pytest.mark.parametrize("chans", [(32, 64), (33, 5), (128, 136)])
@pytest.mark.parametrize("s", [3, 4, 5])
def test_down_exact(gpu, s, chans):
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import encoder_grad as EG
    cin, cout = chans
    k = 2 * s
    rng = np.random.default_rng(1000 * s + cin)
    w, b = _ints(rng, -3, 3, (cout, cin, k)), _ints(rng, -2, 2, (cout,))
    layer = _layer(cin, cout, k, s, 1, DG.ACT_NONE)
    wf, wg = layer.packs(w.to(gpu))
    for T in (1, s - 1, s, s + 1, 2 * s + 1, 129):
        for n in (1, 3):
            x = _ints(rng, -4, 4, (n, cin, T))
            t_out = EG.out_length(T, s)
            dy = _ints(rng, -3, 3, (n, cout, t_out))
            yr, dxr, dwr, dbr = _ref_grads(x, w, b, dy, k, 1, s, False, 1.0, torch.float64)
            assert tuple(yr.shape) == (n, cout, t_out)
            xg, dyg = x.to(gpu), dy.to(gpu)
            y = layer.forward(xg, wf, b.to(gpu))
            assert torch.equal(y.cpu(), yr.float()), f"forward T={T} n={n}"
            dx = layer.grad_input(dyg, xg, tuple(x.shape), wg)
            assert dx.shape == x.shape and torch.equal(dx.cpu(), dxr.float()), f"grad T={T} n={n}"
            dw, db = _wgrad(layer, dyg, xg)
            assert torch.equal(dw.cpu(), dwr.float()) and torch.equal(db.cpu(), dbr.float()), f"wgrad T={T} n={n}"
            assert float(dxr.abs().max()) > 0
        y0 = layer.forward(xg, wf, None)                                   # bias may be null
        assert torch.equal(y0.cpu(), (yr - b.double()[None, :, None]).float())


# (n_items, c_in, c_out, kernel, dilation, stride, T)
WGRAD_CASES = {
    "cout6_cin1": (2, 1, 6, 7, 1, 1, 37),                     # the encoder's first conv; N = 8
    "cout32_cin2_d3": (1, 2, 32, 7, 3, 1, 37),                # the stereo first conv; the 32-row tile
    "cout33_cin33_d9": (2, 33, 33, 7, 9, 1, 37),              # M edge of the 32-row tile; N = 232: a second column tile; T < 54
    "cout64_k1": (1, 32, 64, 1, 1, 1, 50),                    # the residual unit's 1x1; the 64-row tile; N = 33
    "cout72_k3": (2, 64, 72, 3, 1, 1, 40),                    # the projector's kernel; the 64-row tile with an M edge; N = 193
    "cout128_s3": (1, 32, 128, 6, 1, 3, 31),                  # the 128-row tile; strided, ragged
    "cout136_s4": (2, 32, 136, 8, 1, 4, 30),                  # the 128-row tile with an M edge
    "cout64_s5": (1, 32, 64, 10, 1, 5, 23),
    "cout136_cin33_d3": (1, 33, 136, 7, 3, 1, 37),
    "cout128_cin2_d1": (3, 2, 128, 7, 1, 1, 37),
    "red1": (1, 2, 6, 7, 1, 1, 1),                            # reductions around one 32-deep step and its halves
    "red15": (1, 2, 6, 7, 1, 1, 15),
    "red16": (1, 2, 6, 7, 1, 1, 16),
    "red17": (1, 2, 6, 7, 1, 1, 17),
    "red31": (1, 2, 6, 7, 1, 1, 31),
    "red32": (1, 2, 6, 7, 1, 1, 32),
    "red33": (1, 2, 6, 7, 1, 1, 33),
    "items_in_step": (3, 2, 33, 7, 1, 1, 7),                  # three items whose boundaries fall inside one step (T_out = 7)
    "items_in_step_s3": (3, 32, 6, 6, 1, 3, 19),              # the same, strided (T_out = 7)
    "s3_t1": (3, 32, 64, 6, 1, 3, 1),
    "s3_t2": (3, 32, 64, 6, 1, 3, 2),
    "s3_t4": (3, 32, 64, 6, 1, 3, 4),
    "s5_t4": (2, 32, 6, 10, 1, 5, 4),
    "s5_t6": (2, 32, 6, 10, 1, 5, 6),
    "s5_t11": (2, 32, 6, 10, 1, 5, 11),
    "split_1000": (1, 4, 8, 7, 1, 1, 1000),                   # S = 8, the last slice's last step holds 8 of 32 terms
    "split_65531": (1, 4, 8, 7, 1, 1, 65531),                 # S = 512; 65531 terms of magnitude <= 12: the f32 sums are exact
    "split_items": (5, 33, 72, 7, 3, 1, 203),                 # slices that cut through items, two tiles each way
}


@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_wgrad_exact(gpu, name, elu):
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import encoder_grad as EG
    n, cin, cout, k, d, s, T = WGRAD_CASES[name]
    rng = np.random.default_rng(n + cin + cout + k + d + s + T)
    x = _ints(rng, 1, 4, (n, cin, T)) if elu else _ints(rng, -4, 4, (n, cin, T))
    t_out = EG.out_length(T, s)
    dy = _ints(rng, -3, 3, (n, cout, t_out))
    _, S = EG.wgrad_plan(n, cin, T, cout, k, d, s)
    if name.startswith("split"):
        steps = -(-n * t_out // 32)
        per = -(-steps // S)
        assert S >= 3 and (n * t_out - (S - 1) * per * 32) < per * 32      # a last slice that is not full
    _, _, dwr, dbr = _ref_grads(x, torch.zeros(cout, cin, k), torch.zeros(cout), dy, k, d, s, elu, 1.0, torch.float64)
    layer = _layer(cin, cout, k, s, d, DG.ACT_ELU if elu else DG.ACT_NONE)
    dw, db = _wgrad(layer, dy.to(gpu), x.to(gpu))
    assert dw.shape == (cout, cin, k) and db.shape == (cout,) and dw.dtype == torch.float32
    assert torch.equal(dw.cpu(), dwr.float()), f"{name}: dW max diff {float((dw.cpu() - dwr.float()).abs().max())}"
    assert torch.equal(db.cpu(), dbr.float()), f"{name}: db max diff {float((db.cpu() - dbr.float()).abs().max())}"
    dw2, none = _wgrad(layer, dy.to(gpu), x.to(gpu), want_bias=False)     # db may be null
    assert none is None and torch.equal(dw2, dw)
    assert float(dwr.abs().max()) > 0


# ---- B. real values, and ELU's negative side ----
REAL_CASES = ["cout33_cin33_d9", "cout72_k3", "cout128_s3", "cout136_s4", "cout64_s5", "items_in_step", "split_1000", "split_items"]


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", REAL_CASES)
def test_wgrad_elu_negative_side(gpu, name, alpha):
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import encoder_grad as EG
    n, cin, cout, k, d, s, T = WGRAD_CASES[name]
    rng = np.random.default_rng(7 + n + cin + cout + k + d + s + T)
    x = _real(rng, (n, cin, T), 1.5)
    assert float((x < 0).float().mean()) > 0.3
    dy = _real(rng, (n, cout, EG.out_length(T, s)))
    w0, b0 = torch.zeros(cout, cin, k), torch.zeros(cout)
    r64 = _ref_grads(x, w0, b0, dy, k, d, s, True, alpha, torch.float64)
    r32 = _ref_grads(x, w0, b0, dy, k, d, s, True, alpha, torch.float32)
    layer = _layer(cin, cout, k, s, d, DG.ACT_ELU, alpha)
    dw, db = _wgrad(layer, dy.to(gpu), x.to(gpu))
    _bounded(dw, r64[2], r32[2], f"{name} alpha {alpha} dW")
    _bounded(db, r64[3], r32[3], f"{name} alpha {alpha} db")


@pytest.mark.parametrize("s,T,n,cin,cout", [(3, 301, 3, 32, 64), (4, 101, 2, 64, 128), (5, 26, 3, 128, 256), (5, 6, 3, 33, 5)])
def test_down_real_values(gpu, s, T, n, cin, cout):
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import encoder_grad as EG
    k = 2 * s
    rng = np.random.default_rng(s + T + n + cin)
    w, b = _real(rng, (cout, cin, k), 1.0 / np.sqrt(cin * k)), _real(rng, (cout,))
    x, dy = _real(rng, (n, cin, T)), _real(rng, (n, cout, EG.out_length(T, s)))
    r64 = _ref_grads(x, w, b, dy, k, 1, s, False, 1.0, torch.float64)
    r32 = _ref_grads(x, w, b, dy, k, 1, s, False, 1.0, torch.float32)
    layer = _layer(cin, cout, k, s, 1, DG.ACT_NONE)
    wf, wg = layer.packs(w.to(gpu))
    xg, dyg = x.to(gpu), dy.to(gpu)
    _bounded(layer.forward(xg, wf, b.to(gpu)), r64[0], r32[0], f"down s{s} T{T} forward")
    _bounded(layer.grad_input(dyg, xg, tuple(x.shape), wg), r64[1], r32[1], f"down s{s} T{T} grad")
    dw, db = _wgrad(layer, dyg, xg)
    _bounded(dw, r64[2], r32[2], f"down s{s} T{T} dW")
    _bounded(db, r64[3], r32[3], f"down s{s} T{T} db")


# ---- C. whole encoder ----
def _encoder(gpu, model):
    from audiodec_amd import encoder_grad as EG
    enc_tag, pe = MEG.generator_params(model)
    enc = EG.TrainableEncoder(**pe)
    enc.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return enc.to(gpu)


def _generator(gpu, model):
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    enc_tag, pe = MEG.generator_params(model)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return g.eval().to(gpu)


@pytest.mark.parametrize("name", list(MEG.CASES))
def test_encoder_against_reference(gpu, fixture, name):
    model, shape = MEG.CASES[name]
    enc = _encoder(gpu, model)
    x = torch.from_numpy(MEG.case_input(name)).to(gpu).requires_grad_(True)
    z = enc(x)
    z64 = fixture[f"{name}_z64"]
    assert tuple(z.shape) == z64.shape and z.requires_grad
    z.backward(torch.from_numpy(MEG.upstream(int(fixture[f"{name}_seed"]), z64.shape)).to(gpu))
    names = [str(k) for k in fixture[f"{name}_names"]]
    params = dict(enc.named_parameters())
    assert list(params) == names
    got = [z.detach().cpu().numpy().reshape(-1), x.grad.cpu().numpy().reshape(-1)] + \
          [MEG.sample(params[k].grad.cpu().numpy()) for k in names]
    ref = [z64.reshape(-1), fixture[f"{name}_gx64"].reshape(-1)] + [fixture[f"{name}_g{i}"] for i in range(len(names))]
    worst = 0.0
    for what, g, r, e, m in zip(["z", "x"] + names, got, ref, fixture[f"{name}_E_ref"], fixture[f"{name}_max"]):
        assert g.shape == r.shape, what
        err, bound = float(np.abs(g.astype(np.float64) - r).max()), 4 * float(e) + 1e-6 * float(m)
        worst = max(worst, err / bound)
        assert err <= bound, f"{name} {what}: {err:.3e} > {bound:.3e}"
    print(f"encoder {name}: largest err/bound {worst:.3f}")


# ---- D. the denoise step ----
def test_denoise_step(gpu):
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import encoder_grad as EG
    from audiodec_amd import mel
    enc_tag, pe = MEG.generator_params("vctk_sym")
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    gen = _generator(gpu, "vctk_sym")
    dec = DG.FrozenDecoder.from_generator(gen)
    enc = EG.TrainableEncoder.from_generator(gen)
    assert next(enc.parameters()).device == torch.device(gpu)
    loss = mel.MultiMelSpectrogramLoss(fs=48000, device=gpu, differentiable=True)
    B, frames, lam = 2, 4, 0.25                             # the mel loss's largest FFT needs more than 1024 samples
    x = torch.from_numpy(np.stack([synth.synth_audio(11, s, frames * 300) for s in range(B)]))[:, None, :].to(gpu)
    y = torch.from_numpy(np.stack([synth.synth_audio(12, s, frames * 300) for s in range(B)]))[:, None, :].to(gpu)
    params = list(enc.parameters())

    def chain(z):
        zq, vqloss, _ = DG.quantize_st(gen, z)
        return lam * vqloss.sum() + loss(dec(zq), y)

    def step():
        gen_loss = chain(enc(x))
        gen_loss.backward()
        return gen_loss.detach().clone()

    l1 = step()
    g1 = [p.grad.clone() for p in params]
    assert all(g is not None and g.shape == p.shape and bool(torch.isfinite(g).all()) for g, p in zip(g1, params))
    assert all(float(g.abs().max()) > 0 for g in g1)
    # the same values from the encoder's backward alone, dz taken from the chain by hand
    zd = enc(x).detach().requires_grad_(True)
    chain(zd).backward()
    by_hand = torch.autograd.grad(enc(x), params, zd.grad)
    assert all(torch.equal(a, b) for a, b in zip(g1, by_hand))
    # a second backward accumulates (g + g is exact); a second run is bitwise the first
    l2 = step()
    assert torch.equal(l1, l2) and all(torch.equal(p.grad, g + g) for p, g in zip(params, g1))
    enc.zero_grad(set_to_none=True)
    step()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, g1))
    # one optimizer step; the trained weights go back into the streaming generator
    before = [p.detach().clone() for p in params]
    torch.optim.Adam(params, lr=1e-4).step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    with torch.no_grad():
        z_new = enc(x)
        assert not torch.equal(z_new, zd.detach())                      # the packings followed the parameters
    gen.load_state_dict({**sd, **enc.state_dict()})
    gen.configure(num_streams=B, max_frames=3)
    with torch.no_grad():
        z3 = enc(x[:, :, :900])
        z_stream = torch.as_tensor(gen.encode(x[:, :, :900])).clone()     # 2 streams x 3 frames
    assert torch.equal(z3, z_new[:, :, :3])                              # causal: the first frames do not see the last
    err = float((z_stream - z3).abs().max())
    print(f"denoise: streaming encode of the trained weights vs TrainableEncoder {err:.3e} (bound {LATENT_TOL})")
    assert z_stream.shape == z3.shape == (B, 64, 3) and err <= LATENT_TOL


# ---- E. behaviour ----
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


def test_no_grad_frozen_parameters_and_second_backward(gpu):
    enc = _encoder(gpu, "vctk_sym")
    x = torch.from_numpy(MEG.case_input("ragged")).to(gpu)
    up = torch.from_numpy(MEG.upstream(3, (3, 64, 2))).to(gpu)
    names = [k for k, _ in enc.named_parameters()]
    n_convs = sum(1 for k in names if k.endswith("weight"))
    assert n_convs == 30 and len(names) == 34
    z = enc(x)
    assert z.requires_grad and z.grad_fn is not None
    with torch.no_grad():
        z0 = enc(x)
    assert not z0.requires_grad and z0.grad_fn is None and torch.equal(z0, z.detach())        # bitwise the same, nothing saved
    with _Counter("adk_conv_wgrad") as wg, _Counter("adk_dec_conv_grad") as dg:
        z.backward(up)
    assert wg.calls == n_convs and dg.calls == 25           # 24 residual-unit convs and the projector; not the first conv
    full = {k: p.grad.clone() for k, p in enc.named_parameters()}
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        z.backward(up)
    # x requires grad: the first conv's dx is computed too
    enc.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    with _Counter("adk_dec_conv_grad") as dg:
        enc(xg).backward(up)
    assert dg.calls == 26 and xg.grad is not None and float(xg.grad.abs().max()) > 0
    assert all(torch.equal(p.grad, full[k]) for k, p in enc.named_parameters())
    # frozen parameters: no gradient, and no weight-gradient launch
    enc.zero_grad(set_to_none=True)
    frozen = ["encoder.conv_blocks.1.res_units.2.conv1.conv.weight", "encoder.conv_blocks.2.conv.conv.weight", "encoder.conv.conv.weight"]
    for k in frozen:
        enc.get_parameter(k).requires_grad_(False)
    with _Counter("adk_conv_wgrad") as wg:
        enc(x).backward(up)
    assert wg.calls == n_convs - 2                          # block 2's strided conv still owes its bias gradient
    for k, p in enc.named_parameters():
        assert (p.grad is None) if k in frozen else torch.equal(p.grad, full[k]), k
    for p in enc.parameters():
        p.requires_grad_(False)
    assert not enc(x).requires_grad                         # nothing asks for a gradient: no graph
    enc.zero_grad(set_to_none=True)
    xg2 = x.clone().requires_grad_(True)
    with _Counter("adk_conv_wgrad") as wg:
        enc(xg2).backward(up)
    assert wg.calls == 0 and all(p.grad is None for p in enc.parameters())
    assert torch.equal(xg2.grad, xg.grad)                   # the backward to the input does not depend on who is trainable


def test_reproducible_and_stereo(gpu):
    enc = _encoder(gpu, "test_stereo_sym")
    x = torch.from_numpy(MEG.case_input("stereo")).to(gpu)
    up = torch.from_numpy(MEG.upstream(5, (1, 64, 10))).to(gpu)
    runs = []
    for _ in range(2):
        enc.zero_grad(set_to_none=True)
        z = enc(x)
        z.backward(up)
        runs.append([z.detach().clone()] + [p.grad.clone() for p in enc.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert enc.saved_floats(1, 3000) == 3000 * 2 + 7 * (32 * 3000 + 64 * 1000 + 128 * 250 + 256 * 50) + 512 * 10


def test_construction_errors():
    from audiodec_amd import encoder_grad as EG
    for kw, match in (({"use_weight_norm": True}, "weight_g"), ({"mode": "noncausal"}, "causal"),
                      ({"nonlinear_activation": "LeakyReLU"}, "ELU"), ({"codec": "activate_audiodec"}, "ActivateEncoder"),
                      ({"projector": "conv1d_bn"}, "conv1d projector")):
        with pytest.raises(NotImplementedError, match=match):
            EG.TrainableEncoder(**kw)
    _, enc_tag, _, _, _ = configs.alias("vctk_activate_sym")
    _, _, pe = configs.experiment(enc_tag)
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    gen = AutoEncoderStreamGenerator(**pe)
    gen.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    with pytest.raises(NotImplementedError, match="ActivateEncoder"):
        EG.TrainableEncoder.from_generator(gen)
