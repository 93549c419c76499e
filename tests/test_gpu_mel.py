"""GPU: the mel-spectrogram loss (adk_logmel, adk_mel_distance) against the reference and the fp64 restatement.

  * every case of tests/golden/mel.npz: log-mels and losses within 4x the reference's own float32 error against fp64;
  * bitwise reproducibility; MelDistance over batches = one call on their concatenation;
  * Generator.forward's y (vctk_sym) scored against the reference's b3 loss; a lazy-guard decode result as input;
  * TestMain(mel_distance=True) writes mel_distance.txt, and without the flag the output folder is unchanged;
  * a (256, 48000) batch.
"""
import os
import types

import numpy as np
import pytest
import torch

import mel_oracle as MO
from test_mel import mel_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mel.npz"), allow_pickle=False)


def _loss(pname, gpu):
    from audiodec_amd import mel
    return mel.MultiMelSpectrogramLoss(**MO.params(pname), device=gpu)


@pytest.mark.parametrize("pname", list(MO.PARAMS))
def test_cases_against_reference_and_fp64(gpu, fixture, pname):
    p = MO.params(pname)
    loss = _loss(pname, gpu)
    melmats = [fixture[f"{pname}_melmat{r}"] for r in range(len(loss.mel_transfers))]
    for iname in MO.INPUTS:
        y_hat, y = MO.inputs(pname, iname)
        with torch.no_grad():
            got = loss(torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu))
        assert got.dim() == 0 and got.dtype == torch.float32 and got.device.type == "cuda"
        exact = MO.loss64(y_hat, y, p, melmats)
        ref = float(fixture[f"{pname}_{iname}_loss"])
        hip = float(got)
        assert abs(hip - exact) <= 4 * abs(ref - exact) + 1e-7 * abs(exact), f"{pname} {iname}: loss {hip} ref {ref} fp64 {exact}"
        if (pname, iname) in MO.LOGMEL_CASES:
            for r, (f, (n_fft, hop, wl)) in enumerate(zip(loss.mel_transfers, MO.resolutions(p))):
                lm = f(torch.from_numpy(y).to(gpu)).cpu().numpy()
                o = MO.logmel64(y, p["fs"], n_fft, hop, wl, melmats[r], p["eps"], p["log_base"])
                ref_lm = fixture[f"{pname}_{iname}_logmel{r}"]
                assert lm.shape == ref_lm.shape
                bound = 4 * np.max(np.abs(ref_lm - o)) + 1e-6
                err = np.max(np.abs(lm - o))
                assert err <= bound, f"{pname} {iname} r{r}: max|hip - fp64| {err:.3g} > {bound:.3g}"
                assert mel_error(lm, o, p["log_base"]) <= 1e-5, f"{pname} {iname} r{r}: mel error"


def test_layouts_2d_and_3d(gpu):
    loss = _loss("vctk", gpu)
    y_hat, y = MO.inputs("vctk", "synth3")                                 # (3, 1, 9600)
    a, b = torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu)
    l3 = loss(a, b)
    l2 = loss(a.reshape(3, 9600), b.reshape(3, 9600))
    assert torch.equal(l3, l2)
    f = loss.mel_transfers[0]
    assert torch.equal(f(b), f(b.reshape(3, 9600))) and tuple(f(b).shape) == (3, 80, 33)
    stereo = f(b.reshape(1, 3, 9600))                                     # (B, C, T) -> (B*C, T)
    assert torch.equal(stereo, f(b))


def test_nan_propagates(gpu):
    loss = _loss("vctk", gpu)
    y_hat, y = MO.inputs("vctk", "flat2")
    y_hat = y_hat.copy()
    y_hat[0, 1000] = np.nan
    v = loss(torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu))
    assert torch.isnan(v)
    from audiodec_amd import native
    assert native.device_flags() == 0


def test_bitwise_reproducible(gpu):
    loss = _loss("defaults", gpu)
    y_hat, y = (torch.from_numpy(t).to(gpu) for t in MO.inputs("defaults", "synth3"))
    v1, v2 = loss(y_hat, y), loss(y_hat, y)
    assert torch.equal(v1, v2)
    for f in loss.mel_transfers:
        assert torch.equal(f(y), f(y))


def test_mel_distance_over_batches(gpu):
    from audiodec_amd import mel
    y = torch.from_numpy(np.stack([MO._synth((1, 9600), 200 + i)[0] for i in range(8)])).to(gpu)
    y_hat = (y + 0.01 * torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(gpu)).contiguous()
    for pname in ("vctk", "defaults"):
        d = mel.MelDistance(MO.params(pname), gpu)
        for i in range(4):
            d.update(y_hat[2 * i:2 * i + 2], y[2 * i:2 * i + 2])
        one = mel.MelDistance(MO.params(pname), gpu).update(y_hat, y)
        assert d.count() == one.count()
        assert d.value() == pytest.approx(one.value(), rel=1e-12)
        assert d.value() == pytest.approx(float(_loss(pname, gpu)(y_hat, y)), rel=1e-6)
        d.reset()
        assert d.count() == [0] * len(d.loss.mel_transfers) and np.isnan(d.value())


def test_generator_forward_b3(gpu, golden_dir):
    """The vctk_sym Generator.forward output scored against its input: the reference's b3 loss."""
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    from audiodec_amd import configs, synth
    import make_forward_golden as MFG
    fw = np.load(os.path.join(golden_dir, "forward.npz"), allow_pickle=False)
    fx = np.load(os.path.join(golden_dir, "mel.npz"), allow_pickle=False)
    shape, streams = tuple(fw["b3_shape"]), list(fw["b3_streams"])
    x = torch.from_numpy(MFG.forward_input(shape, streams, shape[-1]))
    _, enc_tag, _, _, _ = configs.alias("vctk_sym")
    _, _, pe = configs.experiment(enc_tag)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    g = g.eval().to(gpu).configure(1, 8).set_split16(False).set_offline(True)
    with torch.no_grad():
        y = g.forward(x.to(gpu))[0]
        v = float(_loss("vctk", gpu)(y, x.to(gpu)))
    assert v == pytest.approx(float(fx["b3_loss"]), rel=1e-5)


def test_lazy_guard_result_as_input(gpu, ckpt_root):
    """decode's lazy-guard result gives the same value as a materialised copy of it."""
    from audiodec_amd import lazy_guard, mel
    from audiodec_amd.audiodec import AudioDec, assign_model
    from audiodec_amd import synth
    root = os.path.join(ckpt_root, "mel_lazy")
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
    x = torch.from_numpy(MO._synth((2, 1, 4800), 300)).to(gpu)
    with torch.no_grad():
        y = ad.decoder.decode(ad.rx_encoder.lookup(ad.tx_encoder.quantize(ad.tx_encoder.encode(x))))
        plain = lazy_guard.plain(y).clone()
        loss = _loss("vctk", gpu)
        v_lazy = loss(y, x)
        v_plain = loss(plain, x)
    assert torch.equal(v_lazy, v_plain)
    d = mel.MelDistance(MO.params("vctk"), gpu).update(y, x)
    assert d.value() == pytest.approx(float(v_plain), rel=1e-6)


def _mel_config(path):
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["use_mel_loss"] = True
    cfg["mel_loss_params"] = {k: v for k, v in MO.PARAMS["vctk"].items()}
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)


def test_testmain_mel_distance(gpu, tmp_path):
    from audiodec_amd import configs, mel, offline, synth
    from scipy.io import wavfile
    root = str(tmp_path)
    _, enc, dec = synth.write_model(root, "vctk_sym", 1337)
    _mel_config(os.path.join(os.path.dirname(enc), "config.yml"))
    wavs = os.path.join(root, "wavs")
    os.makedirs(wavs)
    sig = {}
    for i, n in enumerate((4800, 7000)):
        pcm = np.clip(np.rint(MO._synth((n,), 400 + i) * 32767), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(wavs, f"utt{i}.wav"), 48000, pcm)
        sig[f"utt{i}"] = pcm.astype(np.float64) / 32768.0
    outs = {}
    for flag in (False, True):
        args = types.SimpleNamespace(encoder=enc, decoder=dec)
        if flag:
            args.mel_distance = True
        tm = offline.TestMain(args)
        tm.dataset = offline.SingleDataset(files=wavs, query="*.wav", return_utt_id=True)
        tm.load_encoder()
        tm.load_decoder()
        out = os.path.join(root, f"out_{flag}")
        tm.initial_folder("clean_test", out, "True")
        tm.run()
        outs[flag] = (out, tm)
    assert sorted(os.listdir(outs[False][0])) == ["utt0_output.wav", "utt1_output.wav"]
    assert sorted(os.listdir(outs[True][0])) == ["mel_distance.txt", "utt0_output.wav", "utt1_output.wav"]
    lines = open(os.path.join(outs[True][0], "mel_distance.txt")).read().split("\n")
    vals = dict(line.split() for line in lines if line.strip())
    tm = outs[True][1]
    loss = mel.from_config(tm.encoder_config, device=gpu)
    direct = {}
    with torch.no_grad():
        for utt, x in sig.items():
            xt = torch.tensor(x, dtype=torch.float32)[None, None, :].to(gpu)
            y = tm.decode(tm.encode(x[:, None]))[..., :xt.shape[-1]]
            direct[utt] = float(loss(y, xt))
    for utt, v in direct.items():
        assert float(vals[utt]) == pytest.approx(v, rel=1e-6)
    assert float(vals["mean"]) == pytest.approx(np.mean(list(direct.values())), rel=1e-6)
    assert tm.mean_mel_distance == pytest.approx(np.mean(list(direct.values())), rel=1e-6)


def test_large_batch(gpu):
    loss = _loss("vctk", gpu)
    g = torch.Generator(device=gpu).manual_seed(3)
    y = 0.1 * torch.randn(256, 48000, device=gpu, generator=g)
    y_hat = y + 0.01 * torch.randn(256, 48000, device=gpu, generator=g)
    with torch.no_grad():
        v = float(loss(y_hat, y))
    assert np.isfinite(v) and v > 0
    lm = loss.mel_transfers[0](y[:2])
    assert tuple(lm.shape) == (2, 80, 161) and torch.isfinite(lm).all()
    from audiodec_amd import native
    assert native.device_flags() == 0
