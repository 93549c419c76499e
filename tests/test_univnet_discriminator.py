"""CPU: the UnivNet discriminator's host side against tests/golden/univ_disc.npz (made by the unmodified reference).

  * layer tables, output shapes and state-dict keys (the window buffers included) equal what the reference produced;
  * the fp64 restatement (univ_disc_oracle) agrees with the reference's f32 feature maps to f32 round-off, with a bound derived
    from each layer's accumulation length K;
  * loss averaging for every flag combination (AdversarialEval's combination step on fp64 means);
  * the loaders: UnivNet types give the new class, HiFi-GAN types discriminator.Discriminator, unknown types raise;
  * grad-requiring, multi-channel and too-short inputs are rejected before any launch.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

import disc_oracle as DO
import univ_disc_oracle as UO
from audiodec_amd import discriminator as D
from audiodec_amd import synth
from audiodec_amd import univnet_discriminator as U

EPS = 2.0 ** -24                      # f32 unit round-off


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "univ_disc.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def oracle_outs():
    out = {}
    for case, (pname, _) in UO.CASES.items():
        y_hat, y = UO.inputs(case)
        out[case] = UO.forward64(pname, UO.state_dict(pname), np.concatenate([y_hat, y], 0), with_spectrograms=True)
    return out


def test_fixture_records_spectrogram_source(fixture):
    assert int(fixture["torchaudio_real"][0]) in (0, 1)
    assert int(fixture["t_min_rejected"][0]) == UO.T_MIN - 1


@pytest.mark.parametrize("pname", list(UO.PARAMS))
def test_state_dict_keys_equal_the_references(fixture, pname):
    ref_keys = [str(k) for k in fixture[f"keys_{pname}"]]
    d = U.Discriminator(**UO.PARAMS[pname])
    assert sorted(d.state_dict_keys()) == sorted(ref_keys)
    sd = UO.state_dict(pname)
    assert sorted(sd) == sorted(ref_keys)
    for i, (fft, win) in enumerate(zip(UO.PARAMS[pname]["fft_sizes"], UO.PARAMS[pname]["win_lengths"])):
        assert f"mrsd.discriminators.{i}.window" in ref_keys
        assert torch.equal(sd[f"mrsd.discriminators.{i}.window"], torch.hann_window(win))
    spectral = [k for k in ref_keys if k.startswith("mrsd.") and not k.endswith(".window")]
    if pname == "nonorm":
        assert all(k.endswith((".weight", ".bias")) for k in spectral)
    else:
        assert all(k.endswith((".weight_g", ".weight_v", ".bias")) for k in spectral)
    assert f"mrsd.discriminators.{len(UO.PARAMS[pname]['fft_sizes']) - 1}.layers.5.conv.bias" in ref_keys and "mrsd.discriminators.0.layers.0.0.conv.bias" in ref_keys
    d.load_state_dict(sd)                                    # no device: folds on the host only
    with pytest.raises(RuntimeError, match="missing keys"):
        U.Discriminator(**UO.PARAMS[pname]).load_state_dict({k: v for k, v in sd.items() if not k.endswith("1.window")})
    with pytest.raises(ValueError, match="window shape"):
        U.Discriminator(**UO.PARAMS[pname]).load_state_dict(dict(sd, **{"mrsd.discriminators.0.window": torch.ones(7)}))


def test_weight_norm_folding_and_layer_table():
    p = UO.PARAMS["v3"]
    d = U.Discriminator(**p)
    sd = UO.state_dict("v3")
    table = [(L.cin, L.cout, L.kernel, L.stride, L.pad, L.act_slope) for L in d.mrsd.discriminators[0].layers]
    assert table == [(1, 32, (3, 9), (1, 1), (1, 4), 0.2), (32, 32, (3, 9), (1, 2), (1, 4), 0.2), (32, 32, (3, 9), (1, 2), (1, 4), 0.2),
                     (32, 32, (3, 9), (1, 2), (1, 4), 0.2), (32, 32, (3, 3), (1, 1), (1, 1), 0.2), (32, 1, (3, 3), (1, 1), (1, 1), None)]
    L = d.mrsd.discriminators[1].layers[2]
    w = U.effective_weight(sd, L)
    assert torch.equal(w, torch._weight_norm(sd[L.key + ".weight_v"], sd[L.key + ".weight_g"], 0)) and tuple(w.shape) == (32, 32, 3, 9)
    impl = [U.conv_impl(x) for x in d.mrsd.discriminators[0].layers]
    assert impl == [U.IMPL_DIRECT] + [U.IMPL_GEMM] * 4 + [U.IMPL_DIRECT]
    assert d.n_discriminators == 8 and len(d.discriminator_layers) == 8
    assert d.discriminator_layers[3:] == d.mpd.discriminator_layers


def test_layer_plan_matches_fixture_shapes(fixture):
    for case, (pname, (b, c, t)) in UO.CASES.items():
        disc = U.Discriminator(**UO.PARAMS[pname])
        n = 2 * b * c
        for d, sub in enumerate(disc.mrsd.discriminators):
            frames, bins = U.spectrogram_shape(t, sub.fft_size, sub.hop_size, sub.win_length)
            key = f"{case}_spec{d}"
            got = tuple(fixture[key].shape) if key in fixture.files else tuple(fixture[key + "_shape"])
            assert got == (n, frames, bins), f"{case} spec{d}"
            for l, shp in enumerate(sub.output_shapes(n, t)):
                key = f"{case}_d{d}_l{l}"
                got = tuple(fixture[key].shape) if key in fixture.files else tuple(fixture[key + "_shape"])
                assert got == shp, f"{case} d{d} l{l}"
    assert U.spectrogram_shape(48000, 512, 50, 240) == (965, 257)
    assert U.min_samples(512, 240) == UO.T_MIN and U.min_samples(2048, 1200) == 1


def _layer_bound(k, t):
    """The reference's f32 layer against fp64: its input already carries the previous layers' round-off and its own sum is K
    terms long.  With |w| rows of O(1) norm (He scaling) both are below (K + 2) eps max|.| per layer; the chain is at most
    seven stages deep (spectrogram + six convs), and the floor covers maps that are all but zero."""
    return 7 * (k + 2) * EPS * max(1.0, float(np.max(np.abs(t))))


@pytest.mark.parametrize("case", UO.FULL_CASES)
def test_oracle_reproduces_full_cases(fixture, oracle_outs, case):
    outs, specs = oracle_outs[case]
    ks = UO.layer_k(UO.CASES[case][0])
    p = UO.PARAMS[UO.CASES[case][0]]
    assert len(outs) == len(p["fft_sizes"]) + len(p["periods"])
    for i, s in enumerate(specs):
        ref = fixture[f"{case}_spec{i}"]
        assert ref.shape == s.shape
        # an n_fft-point f32 FFT: log2(n_fft) butterfly stages, each a few roundings on values up to max|X|
        n_fft = 2 * (s.shape[-1] - 1)
        err = np.max(np.abs(ref - s))
        assert err <= 4 * np.log2(n_fft) * EPS * max(1.0, np.max(np.abs(s))), f"{case} spec{i}: reference f32 vs fp64 {err:.3g}"
    for d, o in enumerate(outs):
        for l, t in enumerate(o):
            ref = fixture[f"{case}_d{d}_l{l}"]
            assert ref.shape == t.shape, f"{case} d{d} l{l}"
            err = np.max(np.abs(ref - t))
            assert err <= _layer_bound(ks[d][l], t), f"{case} d{d} l{l}: reference f32 vs fp64 {err:.3g}"


def test_oracle_reproduces_v3(fixture, oracle_outs):
    outs, specs = oracle_outs["v3"]
    ks = UO.layer_k("v3")
    for i, s in enumerate(specs):
        assert tuple(fixture[f"v3_spec{i}_shape"]) == s.shape
        n_fft = 2 * (s.shape[-1] - 1)
        err = np.max(np.abs(fixture[f"v3_spec{i}_sample"] - s.reshape(-1)[UO.sample_index(s.size)]))
        assert err <= 4 * np.log2(n_fft) * EPS * max(1.0, np.max(np.abs(s)))
    for d, o in enumerate(outs):
        for l, t in enumerate(o):
            assert tuple(fixture[f"v3_d{d}_l{l}_shape"]) == t.shape
            flat = t.reshape(-1)
            assert np.allclose(fixture[f"v3_d{d}_l{l}_stats"], [flat.mean(), np.abs(flat).mean()], rtol=1e-4, atol=1e-7)
            err = np.max(np.abs(fixture[f"v3_d{d}_l{l}_sample"] - flat[UO.sample_index(flat.size)]))
            assert err <= _layer_bound(ks[d][l], t), f"v3 d{d} l{l}: {err:.3g}"
        assert np.max(np.abs(fixture[f"v3_d{d}_final"] - o[-1])) <= _layer_bound(ks[d][-1], o[-1])


@pytest.mark.parametrize("case", list(UO.CASES))
def test_loss_averaging_all_flags(fixture, oracle_outs, case):
    """AdversarialEval's combination of per-term means, for every flag combination, against the reference's losses."""
    fake, real = UO.split(oracle_outs[case][0])
    disc = U.Discriminator(**UO.PARAMS[UO.CASES[case][0]])
    for gi, (g_avg, g_type) in enumerate(UO.GEN_FLAGS):
        for fi, (fl, fd, ff) in enumerate(UO.FM_FLAGS):
            for use_fm in (True, False):
                ev = D.AdversarialEval(disc, {"average_by_discriminators": g_avg, "loss_type": g_type},
                                       {"average_by_discriminators": g_avg, "loss_type": g_type}, use_fm,
                                       {"average_by_layers": fl, "average_by_discriminators": fd, "include_final_outputs": ff},
                                       lambda_adv=1.5, lambda_feat_match=2.0)
                means = []
                for o_h, o_r in zip(fake, real):
                    f_h, f_r = o_h[-1], o_r[-1]
                    if g_type == "mse":
                        means += [np.mean((f_h - 1) ** 2), np.mean((f_r - 1) ** 2), np.mean(f_h ** 2)]
                    else:
                        means += [np.mean(f_h), np.mean(np.minimum(f_r - 1, 0)), np.mean(np.minimum(-f_h - 1, 0))]
                if use_fm:
                    for o_h, o_r in zip(fake, real):
                        used = len(o_h) if ff else len(o_h) - 1
                        means += [np.mean(np.abs(a - b)) for a, b in zip(o_h[:used], o_r[:used])]
                v = {k: float(x) for k, x in ev._combine(torch.tensor(means, dtype=torch.float64)).items()}
                gen, (r, f) = fixture[f"{case}_gen"][gi], fixture[f"{case}_dis"][gi]
                fmv = fixture[f"{case}_fm"][fi]
                assert v["real_loss"] == pytest.approx(r, rel=1e-5)
                assert v["fake_loss"] == pytest.approx(f, rel=1e-5, abs=1e-7)
                if use_fm:
                    assert v["feature_matching_loss"] == pytest.approx(fmv, rel=1e-5)
                    assert v["adversarial_loss"] == pytest.approx(1.5 * (gen + 2.0 * fmv), rel=1e-5)
                else:
                    assert "feature_matching_loss" not in v
                    assert v["adversarial_loss"] == pytest.approx(1.5 * gen, rel=1e-5)


def test_synth_keeps_hifigan_tensors_and_is_deterministic():
    a, b = synth.discriminator_state_dict(UO.PARAMS["reduced"], 7), synth.discriminator_state_dict(UO.PARAMS["reduced"], 7)
    c = synth.discriminator_state_dict(UO.PARAMS["reduced"], 8)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    # the period half is keyed and scaled as in the HiFi-GAN parameter set
    hifi = synth.discriminator_state_dict(dict(DO.REDUCED, period_discriminator_params=UO.REDUCED["period_discriminator_params"]), 7)
    mpd = [k for k in a if k.startswith("mpd.")]
    assert mpd and all(torch.equal(a[k], hifi[k]) for k in mpd)


@pytest.mark.parametrize("model_type", ["symAudioDecUniv", "UnivNet"])
def test_load_discriminator_univnet(tmp_path, model_type):
    params = UO.PARAMS["reduced"]
    cfg = {"model_type": model_type, "discriminator_params": params, "lambda_adv": 1.0, "use_feat_match_loss": True}
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    ckpt = str(tmp_path / "checkpoint-100steps.pkl")
    torch.save({"model": {"discriminator": UO.state_dict("reduced")}}, ckpt)
    d = U.load_discriminator(ckpt)
    assert type(d) is U.Discriminator and d.config["model_type"] == model_type
    assert [s.fft_size for s in d.mrsd.discriminators] == params["fft_sizes"]
    assert U.from_config(d.config, d).feat_match is not None
    with pytest.raises(NotImplementedError, match=f"Model type: {model_type} is not supported"):
        D.load_discriminator(ckpt)                           # the HiFi-GAN module's loader keeps rejecting these types


@pytest.mark.parametrize("model_type", ["symAudioDec", "HiFiGAN"])
def test_load_discriminator_delegates_hifigan(tmp_path, model_type):
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump({"model_type": model_type, "discriminator_params": DO.PARAMS["reduced"]}, f)
    ckpt = str(tmp_path / "checkpoint-100steps.pkl")
    torch.save({"model": {"discriminator": DO.state_dict("reduced")}}, ckpt)
    assert type(U.load_discriminator(ckpt)) is D.Discriminator
    assert type(U.discriminator_for(model_type, DO.PARAMS["reduced"])) is D.Discriminator


def test_unknown_types_and_arguments_raise():
    with pytest.raises(NotImplementedError, match="Model type: melgan is not supported"):
        U.discriminator_for("melgan", {})
    with pytest.raises(NotImplementedError, match="window"):
        U.Discriminator(window="hamming_window")
    with pytest.raises(NotImplementedError, match="nonlinear_activation"):
        U.Discriminator(spectral_discriminator_params=dict(UO._SPEC, nonlinear_activation="ReLU", nonlinear_activation_params={}))
    with pytest.raises(NotImplementedError, match="fft_size"):
        U.Discriminator(fft_sizes=[1000, 2048, 512])


def test_forward_rejects_before_any_launch():
    d = U.Discriminator(**UO.PARAMS["reduced"]).load_state_dict(UO.state_dict("reduced"))
    with pytest.raises(NotImplementedError, match="forward only"):
        d(torch.zeros(1, 1, 400, requires_grad=True))
    with pytest.raises(ValueError, match="flat_channel"):
        d(torch.zeros(1, 2, 400))
    short = U.Discriminator(**UO.PARAMS["short"]).load_state_dict(UO.state_dict("short"))
    with pytest.raises(ValueError, match="reflect padding"):
        short(torch.zeros(1, 1, UO.T_MIN - 1))
    with pytest.raises(ValueError, match="reflect padding"):
        short(torch.zeros(2, 1, 3))


def test_argument_validation_without_device():
    """Every argument of adk_spectrogram / adk_conv2d is checked before any HIP call: host addresses stand in for device
    pointers, and every call below must fail (or finish) without touching them."""
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    lib = native.lib()
    ARG, SHAPE = -1, -2
    win = np.hanning(512).astype(np.float32)
    Wn, dummy = win.ctypes.data_as(C.c_void_p), C.c_void_p(16)

    def spec(n=2, T=4800, pad=120, n_fft=512, hop=50, wl=240, x=dummy, w=Wn, out=dummy):
        return lib.adk_spectrogram(x, n, T, pad, n_fft, hop, w, wl, out, None)

    for bad in (1000, 128, 8192, 0):
        assert spec(n_fft=bad) == ARG and b"power of two" in lib.adk_last_error()
    assert spec(wl=513) == ARG and spec(wl=0) == ARG and b"win_length" in lib.adk_last_error()
    assert spec(hop=0) == ARG and spec(pad=-1) == ARG and spec(n=-1) == ARG and spec(T=0) == ARG
    assert spec(T=16) == ARG and b"reflect" in lib.adk_last_error()                # 16 + 240 <= 256
    assert spec(w=None) == ARG and spec(x=None) == ARG and spec(out=None) == ARG
    assert spec(out=C.c_void_p(18)) == ARG and b"aligned" in lib.adk_last_error()
    assert spec(n=0, x=None, out=None) == 0                                        # nothing to do: no launch
    assert lib.adk_spectrogram_frames(48000, 120, 50) == 965 and lib.adk_spectrogram_frames(17, 120, 240) == 2
    assert lib.adk_spectrogram_frames(0, 120, 50) == ARG and lib.adk_spectrogram_frames(10, 0, 0) == ARG

    def conv(n=2, cin=32, h=20, w=65, cout=32, kh=3, kw=9, sh=1, sw=2, ph=1, pw=4, act=2, impl=2, x=dummy, wt=dummy, b=dummy, y=dummy):
        return lib.adk_conv2d(x, wt, b, y, n, cin, h, w, cout, kh, kw, sh, sw, ph, pw, act, C.c_float(0.2), impl, None)

    assert conv(n=-1) == ARG and conv(cin=0) == ARG and conv(cout=0) == ARG and conv(h=0) == ARG and conv(w=0) == ARG
    assert conv(kh=0) == ARG and conv(sw=0) == ARG and conv(ph=-1) == ARG
    assert conv(act=1) == ARG and b"act" in lib.adk_last_error()
    assert conv(impl=3) == ARG and conv(impl=0) == ARG and b"impl" in lib.adk_last_error()
    assert conv(h=1, kh=4, ph=1) == SHAPE and conv(w=3, kw=9, pw=2) == SHAPE and b"padded input" in lib.adk_last_error()
    assert conv(cin=512) == ARG and b"4096" in lib.adk_last_error()                 # 512 * 27 taps: beyond the gemm's table
    assert conv(cin=1 << 20, h=1 << 10, w=1 << 10, impl=1) == ARG and b"too large" in lib.adk_last_error()
    assert conv(x=None) == ARG and conv(wt=None) == ARG and conv(y=None) == ARG
    assert conv(y=C.c_void_p(18)) == ARG and conv(b=C.c_void_p(17)) == ARG and b"aligned" in lib.adk_last_error()
    assert conv(n=0, x=None, wt=None, y=None) == 0                                 # nothing to do: no launch
