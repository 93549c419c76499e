"""GPU: the trainable decoder (adk_convtr_wgrad; audiodec_amd/decoder_train.py).

  A. op level, exact: small integer inputs and upstreams make every f32 sum exact, so the transposed conv's weight and bias
     gradients must torch.equal the f64 torch restatement cast to f32 -- with no activation, and with ELU on strictly positive
     inputs (where ELU is the identity) -- over the shapes that can break the indexing, with and without db, on a workspace full
     of NaN;
  B. ELU's negative side and real values: the same op against f64, bound 4 E + 1e-6 max, E the f32 torch CPU error of the same op
     computed here;
  C. whole decoder: every case of decoder_train.npz within 4 E_ref + 1e-6 max of the f64 reference (E_ref the reference's own f32
     error): y, zq.grad and every parameter's sampled gradient;
  D. equivalence with FrozenDecoder (output and dzq, bit for bit), reproducibility, accumulation;
  E. the stage-1 step (encoder, quantizer's straight-through step, decoder, mel loss) and the decoder-only GAN-phase step;
  F. behaviour: launch counts follow needs_input_grad, the second backward, construction errors.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_oracle as DO
import make_decoder_train_golden as MTG
import make_forward_golden as MFG
from audiodec_amd import arch, configs, synth

pytestmark = pytest.mark.gpu
WAVE_TOL = 1e-4


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "decoder_train.npz"), allow_pickle=False)


def _layer(cin, cout, s, act, alpha=1.0):
    from audiodec_amd import decoder_train as DT
    return DT._Layer(arch.ConvSpec("op", "convT", cin, cout, 2 * s, s, 1, 1, True, False), act, alpha)


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def _real(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _convtr_ref(x, w, b, s, act, alpha=1.0):
    """CausalConvTranspose1d.forward (layers/conv_layer.py:189-192) on a(x) for kernel 2s in torch ops (any dtype): replicate padding
    by one frame, the transposed conv, one stride cropped at both ends."""
    h = F.elu(x, alpha) if act else x
    return F.conv_transpose1d(F.pad(h, (1, 0), mode="replicate"), w, b, stride=s)[:, :, s:-s]


def _ref_grads(x, dy, cout, s, act, alpha, dt):
    """(dw, db) of the layer in dtype dt on the CPU (they do not depend on the weights' values)."""
    w = torch.zeros(x.shape[1], cout, 2 * s, dtype=dt, requires_grad=True)
    b = torch.zeros(cout, dtype=dt, requires_grad=True)
    _convtr_ref(x.to(dt), w, b, s, act, alpha).backward(dy.to(dt))
    return w.grad, b.grad


def _bounded(got, ref64, ref32, what):
    """max|got - ref64| <= 4 E + 1e-6 max|ref64|, E = max|ref32 - ref64| (torch's f32 on the CPU)."""
    e, m = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err = float((got.cpu().double() - ref64).abs().max())
    bound = 4 * e + 1e-6 * m
    print(f"{what}: err {err:.3e} E {e:.3e} max {m:.3f} err/bound {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _wgrad(layer, dy, x, want_bias=True):
    """adk_convtr_wgrad through the layer, on a workspace full of NaN (any contents)."""
    from audiodec_amd import decoder_train as DT
    from audiodec_amd import encoder_grad as EG
    s = layer.spec
    ws = EG._Workspace()
    n_bytes, _ = DT.convtr_wgrad_plan(x.shape[0], s.cin, x.shape[2], s.cout, s.k, s.stride)
    ws.get(n_bytes, x.device).fill_(float("nan"))
    return layer.grad_weight(dy, x, ws, want_bias)


# ---- A. op level, exact ----
# (B, T): one frame (only the replicate padding), the step's edge 31 / 32 / 33, and three items' frame-0 terms inside one step
EXACT_SHAPES = [(b, t) for t in (1, 2, 3, 31, 32, 33) for b in (1, 3)] + [(3, 5)]


def _exact(gpu, n, cin, cout, s, T, elu):
    from audiodec_amd import decoder_grad as DG
    rng = np.random.default_rng(1000 * s + 100 * n + T + cin + cout + elu)
    x = _ints(rng, 1, 4, (n, cin, T)) if elu else _ints(rng, -4, 4, (n, cin, T))
    dy = _ints(rng, -3, 3, (n, cout, T * s))
    dwr, dbr = _ref_grads(x, dy, cout, s, elu, 1.0, torch.float64)
    layer = _layer(cin, cout, s, DG.ACT_ELU if elu else DG.ACT_NONE)
    dw, db = _wgrad(layer, dy.to(gpu), x.to(gpu))
    what = f"s{s} B{n} T{T} {cin}->{cout} elu={elu}"
    assert dw.shape == (cin, cout, 2 * s) and db.shape == (cout,) and dw.dtype == torch.float32
    assert torch.equal(dw.cpu(), dwr.float()), f"{what}: dW max diff {float((dw.cpu() - dwr.float()).abs().max())}"
    assert torch.equal(db.cpu(), dbr.float()), f"{what}: db max diff {float((db.cpu() - dbr.float()).abs().max())}"
    dw2, none = _wgrad(layer, dy.to(gpu), x.to(gpu), want_bias=False)     # db may be null
    assert none is None and torch.equal(dw2, dw), what
    assert float(dwr.abs().max()) > 0


@pytest.mark.parametrize("chans", [(64, 32), (33, 5), (136, 128)])
@pytest.mark.parametrize("s", [3, 4, 5])
def test_convtr_wgrad_exact(gpu, s, chans):
    for n, T in EXACT_SHAPES:
        _exact(gpu, n, chans[0], chans[1], s, T, elu=(n + T) % 2 == 1)


def test_convtr_wgrad_exact_split(gpu):
    """S > 1 with a last slice of fewer steps than the others, slices that cut through items, and a reduction that ends inside a
    step: 1050 terms of magnitude <= 24, every f32 partial and their f64 fold exact."""
    from audiodec_amd import decoder_train as DT
    n, cin, cout, s, T = 3, 33, 5, 4, 350
    _, S = DT.convtr_wgrad_plan(n, cin, T, cout, 2 * s, s)
    steps = -(-n * T // 32)
    per = -(-steps // S)
    assert S >= 3 and steps - (S - 1) * per < per and (n * T) % 32
    for elu in (False, True):
        _exact(gpu, n, cin, cout, s, T, elu)


def test_convtr_wgrad_no_items(gpu):
    from audiodec_amd import decoder_grad as DG
    layer = _layer(8, 4, 3, DG.ACT_NONE)
    dw, db = _wgrad(layer, torch.empty(0, 4, 15, device=gpu), torch.empty(0, 8, 5, device=gpu))
    assert not dw.any() and not db.any()                                   # zeros, as adk_conv_wgrad writes them


# ---- B. real values, and ELU's negative side ----
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("s,T,n,cin,cout", [(3, 33, 2, 64, 32), (4, 101, 2, 128, 64), (5, 26, 3, 256, 128), (5, 6, 3, 33, 5),
                                            (4, 1, 3, 40, 7)])
def test_convtr_wgrad_elu_negative_side(gpu, s, T, n, cin, cout, alpha):
    from audiodec_amd import decoder_grad as DG
    rng = np.random.default_rng(7 + s + T + n + cin + cout)
    x = _real(rng, (n, cin, T), 1.5)
    assert float((x < 0).float().mean()) > 0.3
    dy = _real(rng, (n, cout, T * s))
    r64 = _ref_grads(x, dy, cout, s, True, alpha, torch.float64)
    r32 = _ref_grads(x, dy, cout, s, True, alpha, torch.float32)
    dw, db = _wgrad(_layer(cin, cout, s, DG.ACT_ELU, alpha), dy.to(gpu), x.to(gpu))
    _bounded(dw, r64[0], r32[0], f"convtr s{s} T{T} alpha {alpha} dW")
    _bounded(db, r64[1], r32[1], f"convtr s{s} T{T} alpha {alpha} db")


# ---- C. whole decoder ----
def _decoder(gpu, model):
    from audiodec_amd import decoder_train as DT
    enc_tag, pe = MTG.generator_params(model)
    dec = DT.TrainableDecoder(**pe)
    dec.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return dec.to(gpu)


def _frozen(gpu, model):
    from audiodec_amd import decoder_grad as DG
    enc_tag, pe = MTG.generator_params(model)
    dec = DG.FrozenDecoder(pe["code_dim"], pe["output_channels"], pe["decode_channels"], pe["dec_ratios"], pe["dec_strides"], device=gpu)
    return dec.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))


def _generator(gpu, model):
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    enc_tag, pe = MTG.generator_params(model)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return g.eval().to(gpu)


@pytest.mark.parametrize("name", list(MTG.CASES))
def test_decoder_against_reference(gpu, fixture, name):
    model = MTG.CASES[name][0]
    dec = _decoder(gpu, model)
    zq = torch.from_numpy(MTG.case_input(name)).to(gpu).requires_grad_(True)
    y = dec(zq)
    y64 = fixture[f"{name}_y64"]
    assert tuple(y.shape) == y64.shape and y.requires_grad
    y.backward(torch.from_numpy(MTG.upstream(int(fixture[f"{name}_seed"]), y64.shape)).to(gpu))
    names = [str(k) for k in fixture[f"{name}_names"]]
    params = dict(dec.named_parameters())
    assert list(params) == names and len(names) == 34
    got = [y.detach().cpu().numpy().reshape(-1), zq.grad.cpu().numpy().reshape(-1)] + \
          [MTG.sample(params[k].grad.cpu().numpy()) for k in names]
    ref = [y64.reshape(-1), fixture[f"{name}_gzq64"].reshape(-1)] + [fixture[f"{name}_g{i}"] for i in range(len(names))]
    worst, where = 0.0, ""
    for what, g, r, e, m in zip(["y", "zq"] + names, got, ref, fixture[f"{name}_E_ref"], fixture[f"{name}_max"]):
        assert g.shape == r.shape, what
        err, bound = float(np.abs(g.astype(np.float64) - r).max()), 4 * float(e) + 1e-6 * float(m)
        if err / bound > worst:
            worst, where = err / bound, what
        assert err <= bound, f"{name} {what}: {err:.3e} > {bound:.3e}"
    print(f"decoder {name}: largest err/bound {worst:.3f} ({where})")


# ---- D. equivalence, reproducibility, accumulation ----
def test_equals_frozen_decoder_and_reproducible(gpu):
    dec, frozen = _decoder(gpu, "vctk_sym"), _frozen(gpu, "vctk_sym")
    zq_np = MTG.case_input("sym")
    up = torch.from_numpy(MTG.upstream(5, (2, 1, 3300))).to(gpu)
    zf = torch.from_numpy(zq_np).to(gpu).requires_grad_(True)
    yf = frozen(zf)
    yf.backward(up)
    with torch.no_grad():
        y0 = dec(torch.from_numpy(zq_np).to(gpu))
    assert not y0.requires_grad and y0.grad_fn is None and torch.equal(y0, yf.detach())      # bitwise FrozenDecoder's
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        zq = torch.from_numpy(zq_np).to(gpu).requires_grad_(True)
        y = dec(zq)
        y.backward(up)
        runs.append([y.detach().clone(), zq.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(runs[0][0], yf.detach()) and torch.equal(runs[0][1], zf.grad)        # dzq too
    # a second backward accumulates (g + g is exact)
    y = dec(torch.from_numpy(zq_np).to(gpu))
    assert y.requires_grad                                                   # the parameters ask for the graph
    y.backward(up)
    assert all(torch.equal(p.grad, g + g) for p, g in zip(dec.parameters(), runs[0][2:]))
    assert dec.saved_floats(2, 11) == sum(2 * s.cin * t for s, t in zip(dec._specs, _lengths(dec, 11)))


def _lengths(dec, frames):
    t, out = frames, []
    for s in dec._specs:
        out.append(t)
        t *= s.stride if s.kind == "convT" else 1
    return out


# ---- E. the two training steps ----
def _waves(seed, B, n):
    return torch.from_numpy(np.stack([synth.synth_audio(seed, s, n) for s in range(B)]))[:, None, :]


def test_stage1_step(gpu):
    """lambda vqloss.sum() + mel(dec(quantize_st(gen, enc(x))[0]), x): every one of the 68 parameters of encoder, projector and
    decoder gets its gradient; after one Adam step the merged state dict goes back into the streaming generator."""
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import decoder_train as DT
    from audiodec_amd import encoder_grad as EG
    from audiodec_amd import mel
    enc_tag, pe = MTG.generator_params("vctk_sym")
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    gen = _generator(gpu, "vctk_sym")
    enc, dec = EG.TrainableEncoder.from_generator(gen), DT.TrainableDecoder.from_generator(gen)
    assert next(dec.parameters()).device == torch.device(gpu)
    loss = mel.MultiMelSpectrogramLoss(fs=48000, device=gpu, differentiable=True)
    B, frames, lam = 2, 4, 0.25                             # the mel loss's largest FFT needs more than 1024 samples
    x = _waves(11, B, frames * 300).to(gpu)
    params = list(enc.parameters()) + list(dec.parameters())
    assert len(params) == 68

    def step():
        zq, vqloss, _ = DG.quantize_st(gen, enc(x))
        total = lam * vqloss.sum() + loss(dec(zq), x)
        total.backward()
        return total.detach().clone()

    l1 = step()
    g1 = [p.grad.clone() for p in params]
    assert all(g is not None and g.shape == p.shape and bool(torch.isfinite(g).all()) for g, p in zip(g1, params))
    assert all(float(g.abs().max()) > 0 for g in g1)
    for m in (enc, dec):
        m.zero_grad(set_to_none=True)
    assert torch.equal(step(), l1) and all(torch.equal(p.grad, g) for p, g in zip(params, g1))      # bitwise the first run
    before = [p.detach().clone() for p in params]
    torch.optim.Adam(params, lr=1e-4).step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    # the trained weights go back into the streaming generator; its non-streaming lowering (set_offline: the transposed convs see
    # the replicate padding, as Decoder.forward) decodes 2 streams x 3 frames
    with torch.no_grad():
        zq3 = DG.quantize_st(gen, enc(x[:, :, :900]))[0].contiguous()
        y3 = dec(zq3)
        assert not torch.equal(y3, DT.TrainableDecoder.from_generator(gen)(zq3))     # the packings followed the parameters
    gen.load_state_dict({**sd, **enc.state_dict(), **dec.state_dict()})
    gen.set_offline(True)
    gen.configure(num_streams=B, max_frames=3)
    with torch.no_grad():
        y_stream = torch.as_tensor(gen.decode(zq3.transpose(1, 2).contiguous())).clone()
    err = float((y_stream - y3).abs().max())
    print(f"stage 1: the generator's decode of the trained weights vs TrainableDecoder {err:.3e} (bound {WAVE_TOL})")
    assert y_stream.shape == y3.shape == (B, 1, 900) and err <= WAVE_TOL


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


def test_gan_phase_step(gpu):
    """The 'efficient' paradigm's second half: encoder, projector and quantizer frozen, the decoder learns from the generator's
    adversarial loss, which reaches y_hat through the HiFi-GAN discriminator's backward to its input."""
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import decoder_train as DT
    from audiodec_amd import discriminator as D
    from audiodec_amd import encoder_grad as EG
    gen = _generator(gpu, "vctk_sym")
    enc, dec = EG.TrainableEncoder.from_generator(gen), DT.TrainableDecoder.from_generator(gen)
    for p in enc.parameters():
        p.requires_grad_(False)
    disc = D.Discriminator(**DO.PARAMS["reduced"], device=gpu, differentiable=True).load_state_dict(DO.state_dict("reduced"))
    adv = D.GeneratorAdversarialLoss(False, "mse", differentiable=True)
    x = _waves(13, 2, 4 * 300).to(gpu)
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        with _Counter("adk_conv_wgrad") as cw, _Counter("adk_convtr_wgrad") as tw, _Counter("adk_enc_down_grad") as eg:
            z = enc(x)
            assert not z.requires_grad
            zq, _, _ = DG.quantize_st(gen, z)
            assert not zq.requires_grad
            adv(disc(dec(zq))).backward()
        assert (cw.calls, tw.calls, eg.calls) == (26, 4, 0)                # the decoder's 30 convs; nothing of the encoder's
        runs.append([p.grad.clone() for p in dec.parameters()])
    assert len(runs[0]) == 34 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(p.grad is None for p in enc.parameters())


# ---- F. behaviour ----
def test_launch_counts_and_second_backward(gpu):
    dec = _decoder(gpu, "vctk_sym")
    zq_np = MTG.case_input("frame1")
    up = torch.from_numpy(MTG.upstream(3, (3, 1, 300))).to(gpu)
    zq = torch.from_numpy(zq_np).to(gpu)
    y = dec(zq)
    with _Counter("adk_conv_wgrad") as cw, _Counter("adk_convtr_wgrad") as tw, _Counter("adk_dec_conv_grad") as cg, \
            _Counter("adk_dec_convtr_grad") as tg:
        y.backward(up)
    # zq is a constant: conv1's dx is not computed; every other conv's is
    assert (cw.calls, tw.calls, cg.calls, tg.calls) == (26, 4, 25, 4) and zq.grad is None
    full = {k: p.grad.clone() for k, p in dec.named_parameters()}
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        y.backward(up)
    dec.zero_grad(set_to_none=True)
    zg = zq.clone().requires_grad_(True)
    with _Counter("adk_dec_conv_grad") as cg:
        dec(zg).backward(up)
    assert cg.calls == 26 and float(zg.grad.abs().max()) > 0
    assert all(torch.equal(p.grad, full[k]) for k, p in dec.named_parameters())
    # frozen parameters: no gradient, and no weight-gradient launch
    dec.zero_grad(set_to_none=True)
    frozen = ["decoder.conv_blocks.1.res_units.2.conv1.conv.weight", "decoder.conv_blocks.2.conv.deconv.weight",
              "decoder.conv_blocks.3.conv.deconv.weight", "decoder.conv_blocks.3.conv.deconv.bias", "decoder.conv2.conv.weight"]
    for k in frozen:
        dec.get_parameter(k).requires_grad_(False)
    with _Counter("adk_conv_wgrad") as cw, _Counter("adk_convtr_wgrad") as tw:
        dec(zq).backward(up)
    assert (cw.calls, tw.calls) == (24, 3)                  # block 2's transposed conv still owes its bias gradient
    for k, p in dec.named_parameters():
        assert (p.grad is None) if k in frozen else torch.equal(p.grad, full[k]), k
    for p in dec.parameters():
        p.requires_grad_(False)
    assert not dec(zq).requires_grad                        # nothing asks for a gradient: no graph
    dec.zero_grad(set_to_none=True)
    zg2 = zq.clone().requires_grad_(True)
    with _Counter("adk_conv_wgrad") as cw, _Counter("adk_convtr_wgrad") as tw:
        dec(zg2).backward(up)
    assert (cw.calls, tw.calls) == (0, 0) and all(p.grad is None for p in dec.parameters())
    assert torch.equal(zg2.grad, zg.grad)                   # the backward to the input does not depend on who is trainable


def test_stereo_reproducible(gpu):
    dec = _decoder(gpu, "test_stereo_sym")
    zq = torch.from_numpy(MTG.case_input("stereo")).to(gpu)
    up = torch.from_numpy(MTG.upstream(5, (1, 2, 3000))).to(gpu)
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        y = dec(zq)
        y.backward(up)
        runs.append([y.detach().clone()] + [p.grad.clone() for p in dec.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert dec.get_parameter("decoder.conv2.conv.weight").grad.shape == (2, 32, 7)


def test_construction_errors():
    from audiodec_amd import decoder_train as DT
    for kw, match in (({"use_weight_norm": True}, "weight_g"), ({"mode": "noncausal"}, "causal"),
                      ({"nonlinear_activation": "LeakyReLU"}, "ELU"), ({"codec": "activate_audiodec"}, "ActivateDecoder"),
                      ({"kernel_size": 5}, "written for 7")):
        with pytest.raises(NotImplementedError, match=match):
            DT.TrainableDecoder(**kw)
    with pytest.raises(ValueError, match="positive"):
        DT.TrainableDecoder(decode_channels=0)
    _, enc_tag, _, _, _ = configs.alias("vctk_activate_sym")
    _, _, pe = configs.experiment(enc_tag)
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    gen = AutoEncoderStreamGenerator(**pe)
    gen.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    with pytest.raises(NotImplementedError, match="ActivateDecoder"):
        DT.TrainableDecoder.from_generator(gen)
