"""CPU: the HiFi-GAN discriminator's host side against tests/golden/disc.npz (made by the unmodified reference).

  * the fp64 restatement (disc_oracle) reproduces every fixture array within the reference's own f32 error;
  * state-dict layout and weight-norm folding: plain keys in the scale discriminator, g/v in the period discriminator;
  * layer-length planning: the period output conv's H + 1 rows, reflect padding and the AvgPool length;
  * loss averaging for every flag combination (AdversarialEval's combination step on fp64 means);
  * synthetic weights are deterministic; load_discriminator rejects UnivNet; forward rejects grad-requiring inputs.
"""
import os

import numpy as np
import pytest
import torch
import yaml

import disc_oracle as DO
from audiodec_amd import discriminator as D
from audiodec_amd import synth


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "disc.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def oracle_outs():
    out = {}
    for case, (pname, _) in DO.CASES.items():
        y_hat, y = DO.inputs(case)
        out[case] = DO.forward64(pname, DO.state_dict(pname), np.concatenate([y_hat, y], 0))
    return out


def _n_layers(fixture, case, d):
    return len([k for k in fixture.files if k.startswith(f"{case}_d{d}_l") and (k.count("_") == 2 or k.endswith("_shape"))])


@pytest.mark.parametrize("case", DO.FULL_CASES)
def test_oracle_reproduces_full_cases(fixture, oracle_outs, case):
    outs = oracle_outs[case]
    assert len(outs) == 8
    for d, o in enumerate(outs):
        assert len(o) == _n_layers(fixture, case, d)
        for l, t in enumerate(o):
            ref = fixture[f"{case}_d{d}_l{l}"]
            assert ref.shape == t.shape, f"{case} d{d} l{l}"
            err = np.max(np.abs(ref - t))
            assert err <= 2e-6 * max(1.0, np.max(np.abs(t))), f"{case} d{d} l{l}: reference f32 vs fp64 {err:.3g}"


def test_oracle_reproduces_v1(fixture, oracle_outs):
    for d, o in enumerate(oracle_outs["v1"]):
        for l, t in enumerate(o):
            assert tuple(fixture[f"v1_d{d}_l{l}_shape"]) == t.shape
            flat = t.reshape(-1)
            st = fixture[f"v1_d{d}_l{l}_stats"]
            assert np.allclose(st, [flat.mean(), np.abs(flat).mean()], rtol=1e-4, atol=1e-7)
            assert np.max(np.abs(fixture[f"v1_d{d}_l{l}_sample"] - flat[DO.sample_index(flat.size)])) <= 1e-5
        assert np.max(np.abs(fixture[f"v1_d{d}_final"] - o[-1])) <= 1e-5


@pytest.mark.parametrize("case", list(DO.CASES))
def test_oracle_losses(fixture, oracle_outs, case):
    gen, dis, fm = DO.losses64(oracle_outs[case])
    assert np.allclose(fixture[f"{case}_gen"], gen, rtol=1e-5, atol=1e-7)
    assert np.allclose(fixture[f"{case}_dis"], dis, rtol=1e-5, atol=1e-7)
    assert np.allclose(fixture[f"{case}_fm"], fm, rtol=1e-5, atol=1e-7)


def test_state_dict_layout_and_weight_norm():
    p = DO.PARAMS["v1"]
    sd = synth.discriminator_state_dict(p, DO.SEED)
    d = D.Discriminator(**p)
    assert sorted(d.state_dict_keys()) == sorted(sd)
    msd = [k for k in sd if k.startswith("msd.")]
    mpd = [k for k in sd if k.startswith("mpd.")]
    assert msd and all(k.endswith(".weight") or k.endswith(".bias") for k in msd)            # Conv1d: no norm at all
    assert "msd.discriminators.0.layers.0.0.conv.weight" in sd and "msd.discriminators.2.layers.7.conv.bias" in sd
    assert all(k.endswith((".weight_g", ".weight_v", ".bias")) for k in mpd)
    assert "mpd.discriminators.4.output_conv.conv.weight_g" in sd
    assert sum(v.numel() for v in sd.values()) > 70_000_000
    L = [x for x in d._layers if x.key == "mpd.discriminators.1.convs.2.0.conv"][0]
    w = D.effective_weight(sd, L)
    ref = torch._weight_norm(sd[L.key + ".weight_v"], sd[L.key + ".weight_g"], 0).reshape(w.shape)
    assert torch.equal(w, ref) and tuple(w.shape) == (512, 128, 5)
    d.load_state_dict(sd)                                    # no device: folds on the host only
    with pytest.raises(RuntimeError, match="missing keys"):
        D.Discriminator(**p).load_state_dict({k: v for k, v in sd.items() if "output_conv" not in k})
    bad = dict(sd)
    bad["mpd.discriminators.0.convs.0.0.conv.weight_orig"] = bad.pop("mpd.discriminators.0.convs.0.0.conv.weight_g")
    with pytest.raises(NotImplementedError, match="spectral"):
        D.Discriminator(**p).load_state_dict(bad)


def test_layer_plan_matches_fixture_shapes(fixture):
    for case, (pname, (b, c, t)) in DO.CASES.items():
        disc = D.Discriminator(**DO.PARAMS[pname])
        n = 2 * b * c
        shapes = []
        tt = t
        for layers in disc.msd.discriminator_layers:
            h, s = tt, []
            for L in layers:
                h = D.conv_out_len(h, L)
                s.append((n, L.cout, h))
            shapes.append(s)
            tt = D.pool_out_len(tt)
            assert D.pool_out_len(100) == 51
        for p, layers in zip(disc.mpd.periods, disc.mpd.discriminator_layers):
            h, s = (t + D.reflect_pad_len(t, p)) // p, []
            assert (t + D.reflect_pad_len(t, p)) % p == 0
            for L in layers:
                h2 = D.conv_out_len(h, L)
                if L is layers[-1]:
                    assert h2 == h + 1                           # output conv: kernel (2, 1), padding (1, 0)
                    s.append((n, h2 * p))
                else:
                    s.append((n, L.cout, h2, p))
                h = h2
            shapes.append(s)
        for d, s in enumerate(shapes):
            for l, shp in enumerate(s):
                key = f"{case}_d{d}_l{l}"
                got = tuple(fixture[key].shape) if key in fixture.files else tuple(fixture[key + "_shape"])
                assert got == shp, f"{case} d{d} l{l}"
    assert D.reflect_pad_len(1203, 2) == 1 and D.reflect_pad_len(1203, 11) == 7 and D.reflect_pad_len(2310, 7) == 0


def test_impl_choice():
    d = D.Discriminator(**DO.PARAMS["v1"])
    impl = {L.key: D.conv_impl(L) for L in d._layers}
    assert impl["msd.discriminators.0.layers.0.0.conv"] == D.IMPL_DIRECT      # C_in = 1
    assert impl["msd.discriminators.0.layers.7.conv"] == D.IMPL_DIRECT        # C_out = 1
    assert impl["msd.discriminators.0.layers.2.0.conv"] == D.IMPL_GEMM
    assert impl["mpd.discriminators.0.convs.3.0.conv"] == D.IMPL_GEMM


@pytest.mark.parametrize("case", list(DO.CASES))
def test_loss_averaging_all_flags(fixture, oracle_outs, case):
    """AdversarialEval's combination of per-term means, for every flag combination, against the reference's losses."""
    fake, real = DO.split(oracle_outs[case])
    disc = D.Discriminator(**DO.PARAMS[DO.CASES[case][0]])
    for gi, (g_avg, g_type) in enumerate(DO.GEN_FLAGS):
        for fi, (fl, fd, ff) in enumerate(DO.FM_FLAGS):
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


def test_from_config_flags():
    cfg = {"generator_adv_loss_params": {"average_by_discriminators": False},
           "discriminator_adv_loss_params": {"average_by_discriminators": False}, "use_feat_match_loss": True,
           "feat_match_loss_params": {"average_by_discriminators": False, "average_by_layers": False,
                                      "include_final_outputs": False}, "lambda_adv": 1.0, "lambda_feat_match": 2.0}
    ev = D.from_config(cfg, D.Discriminator(**DO.PARAMS["reduced"]))
    assert not ev.gen_adv.average_by_discriminators and ev.gen_adv.loss_type == "mse"
    assert not ev.feat_match.average_by_layers and ev.lambda_feat_match == 2.0
    assert D.from_config(dict(cfg, use_feat_match_loss=False), ev.discriminator).feat_match is None


def test_synthetic_weights_deterministic():
    p = DO.PARAMS["reduced"]
    a, b = synth.discriminator_state_dict(p, 7), synth.discriminator_state_dict(p, 7)
    c = synth.discriminator_state_dict(p, 8)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)


@pytest.mark.parametrize("model_type", ["symAudioDecUniv", "UnivNet"])
def test_load_discriminator_rejects_univnet(tmp_path, model_type):
    with open(tmp_path / "config.yml", "w") as f:
        yaml.safe_dump({"model_type": model_type, "discriminator_params": {}}, f)
    with pytest.raises(NotImplementedError, match=f"Model type: {model_type} is not supported for the discriminator!"):
        D.load_discriminator(str(tmp_path / "checkpoint-100steps.pkl"))


def test_forward_rejects_grad_inputs():
    d = D.Discriminator(**DO.PARAMS["reduced"])
    x = torch.zeros(1, 1, 100, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        d(x)
    with pytest.raises(NotImplementedError, match="forward only"):
        D.GeneratorAdversarialLoss()([[x]])
