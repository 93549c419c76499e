"""GPU: the HiFi-GAN discriminator and GAN eval losses (adk_disc_conv, adk_disc_prep, adk_disc_loss) against the reference and
the fp64 restatement.

  * every case of tests/golden/disc.npz: every feature map within 4x the reference's own float32 error against fp64;
  * the losses under every flag combination to the same bound;
  * bitwise reproducibility; AdversarialEval over two batches = one call on their concatenation = the separate loss classes;
  * a lazy-guard decode result as input;
  * a (16 + 16) x 48000 pass of the shipped architecture, sampled against F.conv* in f64.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_oracle as DO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc.npz"), allow_pickle=False)


_DISCS = {}


def _disc(pname, gpu):
    from audiodec_amd import discriminator as D
    if pname not in _DISCS:
        _DISCS[pname] = D.Discriminator(**DO.PARAMS[pname], device=gpu).load_state_dict(DO.state_dict(pname))
    return _DISCS[pname]


def _x(case, gpu):
    y_hat, y = DO.inputs(case)
    return torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu)


def _bound(ref, exact):
    return 4 * np.max(np.abs(ref - exact)) + 1e-6 * max(1.0, float(np.max(np.abs(exact))))


@pytest.mark.parametrize("case", list(DO.CASES))
def test_feature_maps_against_reference_and_fp64(gpu, fixture, case):
    pname = DO.CASES[case][0]
    a, b = _x(case, gpu)
    x = torch.cat([a, b], 0)
    with torch.no_grad():
        outs = _disc(pname, gpu)(x)
    exact = DO.forward64(pname, DO.state_dict(pname), x.cpu().numpy())
    assert len(outs) == len(exact) == 8
    for d, (o, e) in enumerate(zip(outs, exact)):
        assert len(o) == len(e)
        for l, (t, te) in enumerate(zip(o, e)):
            assert t.device.type == "cuda" and t.dtype == torch.float32
            h = t.cpu().numpy()
            assert h.shape == te.shape, f"{case} d{d} l{l}"
            if case in DO.FULL_CASES:
                ref = fixture[f"{case}_d{d}_l{l}"]
                assert ref.shape == h.shape
                bound, err = _bound(ref, te), np.max(np.abs(h - te))
            else:
                idx = DO.sample_index(te.size)
                ref, ex = fixture[f"{case}_d{d}_l{l}_sample"], te.reshape(-1)[idx]
                bound, err = _bound(ref, ex), np.max(np.abs(h.reshape(-1)[idx] - ex))
            assert err <= bound, f"{case} d{d} l{l}: max|hip - fp64| {err:.3g} > {bound:.3g}"
        if case not in DO.FULL_CASES:
            ref = fixture[f"{case}_d{d}_final"]
            assert np.max(np.abs(o[-1].cpu().numpy() - e[-1])) <= _bound(ref, e[-1])


@pytest.mark.parametrize("case", list(DO.CASES))
def test_losses_all_flags(gpu, fixture, case):
    from audiodec_amd import discriminator as D
    pname = DO.CASES[case][0]
    a, b = _x(case, gpu)
    with torch.no_grad():
        p_, p = _disc(pname, gpu)(a), _disc(pname, gpu)(b)
    gen, dis, fm = DO.losses64(DO.forward64(pname, DO.state_dict(pname), torch.cat([a, b], 0).cpu().numpy()))
    for i, (avg, t) in enumerate(DO.GEN_FLAGS):
        v = float(D.GeneratorAdversarialLoss(avg, t)(p_))
        ref = fixture[f"{case}_gen"][i]
        assert abs(v - gen[i]) <= 4 * abs(ref - gen[i]) + 1e-6 * abs(gen[i]) + 1e-9, f"{case} gen {i}"
        r, f = D.DiscriminatorAdversarialLoss(avg, t)(p_, p)
        for got, k in ((float(r), 0), (float(f), 1)):
            ref = fixture[f"{case}_dis"][i][k]
            assert abs(got - dis[i][k]) <= 4 * abs(ref - dis[i][k]) + 1e-6 * abs(dis[i][k]) + 1e-9, f"{case} dis {i} {k}"
    for i, flags in enumerate(DO.FM_FLAGS):
        v = float(D.FeatureMatchLoss(*flags)(p_, p))
        ref = fixture[f"{case}_fm"][i]
        assert abs(v - fm[i]) <= 4 * abs(ref - fm[i]) + 1e-6 * abs(fm[i]) + 1e-9, f"{case} fm {i}"


def _eval(gpu, pname="reduced", **kw):
    from audiodec_amd import discriminator as D
    cfg = {"generator_adv_loss_params": {"average_by_discriminators": False},
           "discriminator_adv_loss_params": {"average_by_discriminators": False}, "use_feat_match_loss": True,
           "feat_match_loss_params": {"average_by_discriminators": False, "average_by_layers": False,
                                      "include_final_outputs": False}, "lambda_adv": 1.0, "lambda_feat_match": 2.0}
    cfg.update(kw)
    return D.from_config(cfg, _disc(pname, gpu))


def test_bitwise_reproducible(gpu):
    a, b = _x("t1203", gpu)
    d = _disc("reduced", gpu)
    with torch.no_grad():
        o1, o2 = d(torch.cat([a, b])), d(torch.cat([a, b]))
        v1, v2 = _eval(gpu)(a, b), _eval(gpu)(a, b)
    assert all(torch.equal(x, y) for p, q in zip(o1, o2) for x, y in zip(p, q))
    assert all(torch.equal(v1[k], v2[k]) for k in v1)


def test_adversarial_eval_batches_and_classes(gpu, fixture):
    from audiodec_amd import discriminator as D
    a1, b1 = _x("t1203", gpu)
    g = torch.Generator(device=gpu).manual_seed(11)
    a2 = (0.1 * torch.randn(2, 1, 1203, device=gpu, generator=g)).contiguous()
    b2 = (0.1 * torch.randn(2, 1, 1203, device=gpu, generator=g)).contiguous()
    ev = _eval(gpu)
    with torch.no_grad():
        ev.update(a1, b1).update(a2, b2)
        whole = ev.forward(torch.cat([a1, a2]), torch.cat([b1, b2]))
    got = ev.value()
    assert set(got) == {"adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss"}
    for k in got:
        assert got[k] == pytest.approx(float(whole[k]), rel=1e-6)
    # one batch against the separate loss classes on forward outputs, and against the reference's numbers (flag set 0)
    with torch.no_grad():
        v = ev.forward(a1, b1)
        d = _disc("reduced", gpu)
        p_, p = d(a1), d(b1)
        adv = D.GeneratorAdversarialLoss(False)(p_)
        fm = D.FeatureMatchLoss(False, False, False)(p_, p)
        r, f = D.DiscriminatorAdversarialLoss(False)(p_, p)
    assert float(v["feature_matching_loss"]) == pytest.approx(float(fm), rel=1e-6)
    assert float(v["adversarial_loss"]) == pytest.approx(float(adv) + 2.0 * float(fm), rel=1e-6)
    assert float(v["real_loss"]) == pytest.approx(float(r), rel=1e-6)
    assert float(v["fake_loss"]) == pytest.approx(float(f), rel=1e-6)
    assert float(v["feature_matching_loss"]) == pytest.approx(float(fixture["t1203_fm"][0]), rel=1e-5)
    assert float(v["real_loss"]) == pytest.approx(float(fixture["t1203_dis"][0][0]), rel=1e-5)
    ev.reset()
    assert ev.update(a1, b1).value()["fake_loss"] == pytest.approx(float(fixture["t1203_dis"][0][1]), rel=1e-5)


def test_lazy_guard_result_as_input(gpu, ckpt_root):
    from audiodec_amd import lazy_guard, synth
    from audiodec_amd.audiodec import AudioDec, assign_model
    root = os.path.join(ckpt_root, "disc_lazy")
    os.makedirs(root, exist_ok=True)
    synth.write_model(root, "vctk_sym", 1337)
    cwd = os.getcwd()
    os.chdir(root)
    try:
        _, enc, dec = assign_model("vctk_sym")
        ad = AudioDec(tx_device=gpu, rx_device=gpu, num_streams=2, max_frames=16)
        ad.load_transmitter(enc)
        ad.load_receiver(enc, dec)
    finally:
        os.chdir(cwd)
    x = torch.from_numpy(np.stack([synth.synth_audio(3, s, 4800) for s in range(2)]))[:, None].to(gpu)
    with torch.no_grad():
        y = ad.decoder.decode(ad.rx_encoder.lookup(ad.tx_encoder.quantize(ad.tx_encoder.encode(x))))
        plain = lazy_guard.plain(y).clone()
        ev = _eval(gpu)
        v_lazy, v_plain = ev(y, x), ev(plain, x)
    assert all(torch.equal(v_lazy[k], v_plain[k]) for k in v_lazy)


def test_shipped_architecture_eval_shape(gpu):
    """(16 + 16) x 48000 with the shipped architecture: runs, and sampled layers match F.conv* in f64 on their HIP input."""
    sd = DO.state_dict("v1")
    d = _disc("v1", gpu)
    g = torch.Generator(device=gpu).manual_seed(2)
    y = (0.1 * torch.randn(16, 1, 48000, device=gpu, generator=g)).clamp(-1, 1).contiguous()
    y_hat = (y + 0.02 * torch.randn(16, 1, 48000, device=gpu, generator=g)).contiguous()
    x = torch.cat([y_hat, y])
    with torch.no_grad():
        vals = _eval(gpu, "v1")(y_hat, y)
        outs = d(x)
    assert all(torch.isfinite(v) for v in vals.values())
    rows = torch.tensor([0, 17, 31], device=gpu)
    subs = d.msd.discriminator_layers + d.mpd.discriminator_layers
    for di in (0, 2, 3, 7):                                  # scales 1 and 3, periods 2 and 11
        layers = subs[di]
        for l in range(1, len(layers)):
            L = layers[l]
            w, b = DO._weight64(sd, L)
            w, b = w.to(gpu), b.to(gpu)
            inp = outs[di][l - 1].index_select(0, rows).double()
            if L.conv2d:
                ref = F.conv2d(inp, w, b, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups)
            else:
                ref = F.conv1d(inp, w, b, stride=L.stride, padding=L.pad, groups=L.groups)
            if L.act_slope is not None:
                ref = F.leaky_relu(ref, L.act_slope)
            got = outs[di][l].index_select(0, rows).double().reshape(ref.shape)
            # f32 accumulation over K = (C_in / g) * k terms: at most K u sum |w x| (u = 2^-24), plus the bias add
            mag = (F.conv2d(inp.abs(), w.abs(), None, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups) if L.conv2d
                   else F.conv1d(inp.abs(), w.abs(), None, stride=L.stride, padding=L.pad, groups=L.groups))
            k = (L.cin // L.groups) * L.kernel
            assert torch.all((got - ref).abs() <= (k + 2) * 2.0 ** -24 * (mag + b.abs().max()) + 1e-7), f"d{di} l{l}"
