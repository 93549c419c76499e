"""GPU: the UnivNet discriminator (adk_spectrogram, adk_conv2d + the period half and losses of disc.hip) against the reference
and the fp64 restatement.

  * every case of tests/golden/univ_disc.npz: every feature map, and the spectrogram through the raw entry point, within 4x the
    reference's own float32 error against fp64; the losses under every flag combination to the same bound;
  * bitwise reproducibility; AdversarialEval over two batches = one call on their concatenation = the separate loss classes;
  * a lazy-guard decode result of a vctk_univ_sym model as input;
  * a (16 + 16) x 48000 pass of the shipped architecture: the spectrograms sampled against an f64 rFFT and every spectral
    layer, the first included, sampled against F.conv2d in f64; raw adk_conv2d calls that span several tile rows.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import univ_disc_oracle as UO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "univ_disc.npz"), allow_pickle=False)


_DISCS = {}


def _disc(pname, gpu):
    from audiodec_amd import univnet_discriminator as U
    if pname not in _DISCS:
        _DISCS[pname] = U.Discriminator(**UO.PARAMS[pname], device=gpu).load_state_dict(UO.state_dict(pname))
    return _DISCS[pname]


def _x(case, gpu):
    y_hat, y = UO.inputs(case)
    return torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu)


def _bound(ref, exact):
    return 4 * np.max(np.abs(ref - exact)) + 1e-6 * max(1.0, float(np.max(np.abs(exact))))


@pytest.mark.parametrize("case", list(UO.CASES))
def test_spectrogram_entry_point(gpu, fixture, case):
    from audiodec_amd import univnet_discriminator as U
    pname = UO.CASES[case][0]
    a, b = _x(case, gpu)
    x = torch.cat([a, b], 0)
    x = x.reshape(-1, x.shape[-1]).contiguous()
    sd = UO.state_dict(pname)
    _, exact = UO.forward64(pname, sd, torch.cat([a, b], 0).cpu().numpy(), with_spectrograms=True)
    d = _disc(pname, gpu)
    for i, sub in enumerate(d.mrsd.discriminators):
        got = U.spectrogram(x, sd[sub.window_key].to(gpu), sub.fft_size, sub.hop_size, sub.win_length)
        torch.cuda.synchronize()
        h, e = got.cpu().numpy(), exact[i]
        assert h.shape == e.shape and got.dtype == torch.float32
        if case in UO.FULL_CASES:
            ref = fixture[f"{case}_spec{i}"]
            bound, err = _bound(ref, e), np.max(np.abs(h - e))
        else:
            idx = UO.sample_index(e.size)
            ref, ex = fixture[f"{case}_spec{i}_sample"], e.reshape(-1)[idx]
            bound, err = _bound(ref, ex), np.max(np.abs(h.reshape(-1)[idx] - ex))
        print(f"{case} spec{i}: max|hip - fp64| {err:.3g}  bound {bound:.3g}")
        assert err <= bound, f"{case} spec{i}: max|hip - fp64| {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("case", list(UO.CASES))
def test_feature_maps_against_reference_and_fp64(gpu, fixture, case):
    pname = UO.CASES[case][0]
    a, b = _x(case, gpu)
    x = torch.cat([a, b], 0)
    with torch.no_grad():
        outs = _disc(pname, gpu)(x)
    exact = UO.forward64(pname, UO.state_dict(pname), x.cpu().numpy())
    assert len(outs) == len(exact) == len(UO.PARAMS[pname]["fft_sizes"]) + len(UO.PARAMS[pname]["periods"])
    for d, (o, e) in enumerate(zip(outs, exact)):
        assert len(o) == len(e)
        for l, (t, te) in enumerate(zip(o, e)):
            assert t.device.type == "cuda" and t.dtype == torch.float32
            h = t.cpu().numpy()
            assert h.shape == te.shape, f"{case} d{d} l{l}"
            if case in UO.FULL_CASES:
                ref = fixture[f"{case}_d{d}_l{l}"]
                assert ref.shape == h.shape
                bound, err = _bound(ref, te), np.max(np.abs(h - te))
            else:
                idx = UO.sample_index(te.size)
                ref, ex = fixture[f"{case}_d{d}_l{l}_sample"], te.reshape(-1)[idx]
                bound, err = _bound(ref, ex), np.max(np.abs(h.reshape(-1)[idx] - ex))
            print(f"{case} d{d} l{l}: max|hip - fp64| {err:.3g}  bound {bound:.3g}")
            assert err <= bound, f"{case} d{d} l{l}: max|hip - fp64| {err:.3g} > {bound:.3g}"
        if case not in UO.FULL_CASES:
            ref = fixture[f"{case}_d{d}_final"]
            assert np.max(np.abs(o[-1].cpu().numpy() - e[-1])) <= _bound(ref, e[-1])


@pytest.mark.parametrize("case", list(UO.CASES))
def test_losses_all_flags(gpu, fixture, case):
    from audiodec_amd import discriminator as D
    pname = UO.CASES[case][0]
    a, b = _x(case, gpu)
    with torch.no_grad():
        p_, p = _disc(pname, gpu)(a), _disc(pname, gpu)(b)
    gen, dis, fm = UO.losses64(UO.forward64(pname, UO.state_dict(pname), torch.cat([a, b], 0).cpu().numpy()))
    for i, (avg, t) in enumerate(UO.GEN_FLAGS):
        v = float(D.GeneratorAdversarialLoss(avg, t)(p_))
        ref = fixture[f"{case}_gen"][i]
        assert abs(v - gen[i]) <= 4 * abs(ref - gen[i]) + 1e-6 * abs(gen[i]) + 1e-9, f"{case} gen {i}"
        r, f = D.DiscriminatorAdversarialLoss(avg, t)(p_, p)
        for got, k in ((float(r), 0), (float(f), 1)):
            ref = fixture[f"{case}_dis"][i][k]
            assert abs(got - dis[i][k]) <= 4 * abs(ref - dis[i][k]) + 1e-6 * abs(dis[i][k]) + 1e-9, f"{case} dis {i} {k}"
    for i, flags in enumerate(UO.FM_FLAGS):
        v = float(D.FeatureMatchLoss(*flags)(p_, p))
        ref = fixture[f"{case}_fm"][i]
        assert abs(v - fm[i]) <= 4 * abs(ref - fm[i]) + 1e-6 * abs(fm[i]) + 1e-9, f"{case} fm {i}"


_CFG = {"generator_adv_loss_params": {"average_by_discriminators": False},
        "discriminator_adv_loss_params": {"average_by_discriminators": False}, "use_feat_match_loss": True,
        "feat_match_loss_params": {"average_by_discriminators": False, "average_by_layers": False,
                                   "include_final_outputs": False}, "lambda_adv": 1.0, "lambda_feat_match": 2.0}


def _eval(gpu, pname="reduced", **kw):
    from audiodec_amd import discriminator as D
    return D.from_config(dict(_CFG, **kw), _disc(pname, gpu))


def test_bitwise_reproducible(gpu):
    a, b = _x("t301", gpu)
    d = _disc("reduced", gpu)
    with torch.no_grad():
        o1, o2 = d(torch.cat([a, b])), d(torch.cat([a, b]))
        v1, v2 = _eval(gpu)(a, b), _eval(gpu)(a, b)
    assert all(torch.equal(x, y) for p, q in zip(o1, o2) for x, y in zip(p, q))
    assert all(torch.equal(v1[k], v2[k]) for k in v1)


def test_adversarial_eval_batches_and_classes(gpu, fixture):
    from audiodec_amd import discriminator as D
    a1, b1 = _x("t301", gpu)
    g = torch.Generator(device=gpu).manual_seed(11)
    a2 = (0.1 * torch.randn(2, 1, 301, device=gpu, generator=g)).contiguous()
    b2 = (0.1 * torch.randn(2, 1, 301, device=gpu, generator=g)).contiguous()
    ev = _eval(gpu)
    with torch.no_grad():
        ev.update(a1, b1).update(a2, b2)
        whole = ev.forward(torch.cat([a1, a2]), torch.cat([b1, b2]))
    got = ev.value()
    assert set(got) == {"adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss"}
    for k in got:
        assert got[k] == pytest.approx(float(whole[k]), rel=1e-6)
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
    assert float(v["feature_matching_loss"]) == pytest.approx(float(fixture["t301_fm"][0]), rel=1e-5)
    assert float(v["real_loss"]) == pytest.approx(float(fixture["t301_dis"][0][0]), rel=1e-5)
    ev.reset()
    assert ev.update(a1, b1).value()["fake_loss"] == pytest.approx(float(fixture["t301_dis"][0][1]), rel=1e-5)


def test_stereo_flat_channel_eval(gpu, fixture):
    a, b = _x("stereo", gpu)
    with torch.no_grad():
        v = _eval(gpu, "flat")(a, b)
    assert float(v["feature_matching_loss"]) == pytest.approx(float(fixture["stereo_fm"][0]), rel=1e-5)
    assert float(v["real_loss"]) == pytest.approx(float(fixture["stereo_dis"][0][0]), rel=1e-5)
    assert float(v["fake_loss"]) == pytest.approx(float(fixture["stereo_dis"][0][1]), rel=1e-5)


def test_lazy_guard_result_as_input(gpu, ckpt_root):
    from audiodec_amd import lazy_guard, synth
    from audiodec_amd.audiodec import AudioDec, assign_model
    root = os.path.join(ckpt_root, "univ_disc_lazy")
    os.makedirs(root, exist_ok=True)
    synth.write_model(root, "vctk_univ_sym", 1337)
    cwd = os.getcwd()
    os.chdir(root)
    try:
        _, enc, dec = assign_model("vctk_univ_sym")
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
    """(16 + 16) x 48000 with the shipped parameters: runs, is finite; sampled rows of the spectrogram match an f64 rFFT, and
    sampled rows of every spectral layer (the first included) match F.conv2d in f64 on their own HIP input."""
    from audiodec_amd import univnet_discriminator as U
    sd = UO.state_dict("v3")
    d = _disc("v3", gpu)
    g = torch.Generator(device=gpu).manual_seed(2)
    y = (0.1 * torch.randn(16, 1, 48000, device=gpu, generator=g)).clamp(-1, 1).contiguous()
    y_hat = (y + 0.02 * torch.randn(16, 1, 48000, device=gpu, generator=g)).contiguous()
    with torch.no_grad():
        vals = _eval(gpu, "v3")(y_hat, y)
    assert all(torch.isfinite(v) for v in vals.values())
    rows = torch.tensor([0, 17, 31], device=gpu)
    x = torch.cat([y_hat, y])
    for di, sub in enumerate(d.mrsd.discriminators):
        with torch.no_grad():
            # the layers' own input at this size, through the raw entry point, against the fp64 restatement's rFFT
            spec = U.spectrogram(x[:, 0].contiguous(), sd[sub.window_key].to(gpu), sub.fft_size, sub.hop_size, sub.win_length)
            assert tuple(spec.shape) == (32,) + U.spectrogram_shape(48000, sub.fft_size, sub.hop_size, sub.win_length)
            e = UO.spectrogram64(x[:, 0].index_select(0, rows).double().cpu(), sd[sub.window_key].double(), sub.fft_size,
                                 sub.hop_size, sub.win_length)
            got = spec.index_select(0, rows).double().cpu()
            # an f32 FFT of n_fft points: log2(n_fft) stages of a few roundings each on values up to max|X|, then |.|
            tol = 4 * np.log2(sub.fft_size) * 2.0 ** -24 * max(1.0, float(e.abs().max()))
            err = float((got - e).abs().max())
            print(f"spec{di} at 32 x 48000: max|hip - fp64| {err:.3g}  bound {tol:.3g}")
            assert err <= tol, f"spec{di}: {err:.3g} > {tol:.3g}"
            prev = spec[:, None]
            for _, l, t, _ in sub.layers_of(x):                              # one resolution at a time: ~2 GB of maps
                if l == 0:
                    assert torch.equal(t, d._convs[sub.layers[0].key](prev))    # the pass computed layer 0 from this spectrogram
                L = sub.layers[l]
                w, b = UO._weight64(sd, L)
                w, b = w.to(gpu), b.to(gpu)
                inp = prev.index_select(0, rows).double()
                ref = F.conv2d(inp, w, b, stride=L.stride, padding=L.pad)
                if L.act_slope is not None:
                    ref = F.leaky_relu(ref, L.act_slope)
                got = t.index_select(0, rows).double()
                assert got.shape == ref.shape
                # f32 accumulation over K = C_in * kh * kw terms: at most K u sum |w x| (u = 2^-24), plus the bias add
                mag = F.conv2d(inp.abs(), w.abs(), None, stride=L.stride, padding=L.pad)
                k = L.cin * L.kernel[0] * L.kernel[1]
                assert torch.all((got - ref).abs() <= (k + 2) * 2.0 ** -24 * (mag + b.abs().max()) + 1e-7), f"d{di} l{l}"
                prev = t
            assert torch.isfinite(prev).all()


def test_conv2d_gemm_several_tile_rows(gpu):
    """adk_conv2d's GEMM with C_out > 32 (two grid rows of the 32 x 128 tile, the second partly filled), K not a multiple of
    16, strides and paddings on both axes, against F.conv2d in f64; and the direct kernel with C_out not a multiple of 8."""
    from audiodec_amd import univnet_discriminator as U
    g = torch.Generator(device=gpu).manual_seed(5)
    for cin, cout, kernel, stride, pad, slope in ((5, 40, (3, 5), (2, 3), (1, 2), 0.2), (3, 70, (2, 3), (1, 2), (1, 0), None),
                                                 (1, 11, (3, 9), (1, 2), (1, 4), 0.2), (6, 1, (3, 3), (2, 1), (0, 1), None)):
        L = U.SpecLayer("t", cin, cout, kernel, stride, pad, True, slope, "none")
        w = torch.randn(cout, cin, *kernel, device=gpu, generator=g) / (cin * kernel[0] * kernel[1]) ** 0.5
        b = torch.randn(cout, device=gpu, generator=g)
        x = torch.randn(3, cin, 37, 53, device=gpu, generator=g).contiguous()
        conv = U._Conv2d(L, w.cpu(), b.cpu(), gpu)
        assert conv.impl == (U.IMPL_DIRECT if cin == 1 or cout == 1 else U.IMPL_GEMM)
        got = conv(x).double()
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
        if slope is not None:
            ref = F.leaky_relu(ref, slope)
        assert got.shape == ref.shape
        mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=pad)
        k = cin * kernel[0] * kernel[1]
        assert torch.all((got - ref).abs() <= (k + 2) * 2.0 ** -24 * (mag + b.abs().max()) + 1e-7), f"{cin} -> {cout} {kernel}"
