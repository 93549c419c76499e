"""GPU: the STFT loss (adk_stft_mag, adk_stft_distance, adk_mag_distance) and the waveform-shape loss (adk_shape_distance)
against the reference's float32 values (tests/golden/stft_loss.npz) and the fp64 restatement (stft_oracle).

  * losses of every (parameter set, input): with e(v) = |v - fp64| / |fp64|, e(hip) <= 4 max(e(ref of the case), E), E the
    largest e(ref) over the ordinary inputs of the same parameter set and term, computed from the fixture;
  * magnitudes of the stored cases: max |hip - fp64| <= 4 max |ref - fp64| + 1e-6, and per frame
    |hip - fp64| / max_k fp64 <= 1e-5; stft() fed through the two magnitude losses equals the fused path to rel 1e-6;
  * shape loss: |hip - fp64| <= 4 |ref - fp64| + 2.4e-7 |fp64| -- 2^-22: every |a - b| is one f32 subtraction of exact maxima
    (relative error <= 2^-24), the sum is f64, and one rounding to f32 ends it (2^-24), with a factor two to spare; the
    all-(+-1) input is exactly 0;
  * the grid-stride paths, bitwise reproducibility, layouts, NaN, the accumulators, a lazy-guard input, the offline driver.
"""
import os
import types

import numpy as np
import pytest
import torch

import mel_oracle as MO
import stft_oracle as SO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "stft_loss.npz"), allow_pickle=False)


def _loss(pname, gpu):
    from audiodec_amd import stft_loss
    return stft_loss.MultiResolutionSTFTLoss(**SO.PARAMS[pname], device=gpu)


def _pair(pname, iname, gpu):
    return tuple(torch.from_numpy(a).to(gpu) for a in SO.inputs(pname, iname))


def rel(v, exact):
    return abs(float(v) - exact) / abs(exact)


@pytest.mark.parametrize("pname", list(SO.PARAMS))
def test_losses_against_reference_and_fp64(gpu, fixture, pname):
    loss = _loss(pname, gpu)
    e_ref = {(i, t): rel(fixture[f"{pname}_{i}_{t}"], SO.exact_loss(pname, i)[k])
             for i in SO.INPUTS for k, t in enumerate(("sc", "mag"))}
    floor = {t: max(e_ref[i, t] for i in SO.ORDINARY) for t in ("sc", "mag")}
    failures = []
    for iname in SO.INPUTS:
        x, y = _pair(pname, iname, gpu)
        with torch.no_grad():
            got = loss(x, y)
        assert len(got) == 2
        for k, t in enumerate(("sc", "mag")):
            assert got[k].dim() == 0 and got[k].dtype == torch.float32 and got[k].device.type == "cuda"
            exact = SO.exact_loss(pname, iname)[k]
            e_hip, bound = rel(got[k], exact), 4 * max(e_ref[iname, t], floor[t])
            print(f"{pname} {iname} {t}: hip {float(got[k]):.9g} fp64 {exact:.9g} e(hip) {e_hip:.3g} e(ref) {e_ref[iname, t]:.3g} "
                  f"E {floor[t]:.3g} bound {bound:.3g}")
            if not e_hip <= bound:
                failures.append(f"{pname} {iname} {t}: e(hip) {e_hip:.3g} > {bound:.3g}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("case", SO.MAG_CASES, ids=lambda c: "-".join(c))
def test_magnitudes(gpu, fixture, case):
    from audiodec_amd import stft_loss
    pname, iname = case
    p = SO.PARAMS[pname]
    loss = _loss(pname, gpu)
    x, y = _pair(pname, iname, gpu)
    x2, y2 = x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1])
    for r, (f, (n_fft, hop, wl)) in enumerate(zip(loss.stft_losses, SO.resolutions(p))):
        ym = stft_loss.stft(y2, n_fft, hop, wl, f.window)
        assert ym.dtype == torch.float32 and tuple(ym.shape) == (y2.shape[0], 1 + y2.shape[-1] // hop, n_fft // 2 + 1)
        assert ym.is_contiguous()
        o = SO.mag64(y2.cpu().numpy(), n_fft, hop, wl, SO.window_f32(p["window"], wl))
        ref = fixture[f"{pname}_{iname}_ymag{r}"]
        hip = ym.cpu().numpy()
        err, bound = np.max(np.abs(hip - o)), 4 * np.max(np.abs(ref - o)) + 1e-6
        frame_err = np.max(np.abs(hip - o) / o.max(axis=-1, keepdims=True))
        print(f"{pname} {iname} r{r}: max|hip - fp64| {err:.3g} (bound {bound:.3g})  per-frame relative {frame_err:.3g}")
        assert err <= bound, f"{pname} {iname} r{r}: max|hip - fp64| {err:.3g} > {bound:.3g}"
        assert frame_err <= 1e-5, f"{pname} {iname} r{r}"
        # the magnitude losses on stft()'s output against the fused kernel
        xm = stft_loss.stft(x2, n_fft, hop, wl, f.window)
        sc, mag = f(x2, y2)
        assert float(stft_loss.SpectralConvergenceLoss()(xm, ym)) == pytest.approx(float(sc), rel=1e-6)
        assert float(stft_loss.LogSTFTMagnitudeLoss()(xm, ym)) == pytest.approx(float(mag), rel=1e-6)


def test_shape_loss_against_reference_and_fp64(gpu, fixture):
    from audiodec_amd import waveform_loss
    failures = []
    for iname in SO.SHAPE_INPUTS:
        y_hat, y = SO.inputs("defaults", iname)
        a, b = torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu)
        for wname in SO.SHAPE_WINLENS:
            winlens = SO.shape_winlens(wname, y.shape[-1])
            got = waveform_loss.MultiWindowShapeLoss(winlens)(a, b)
            assert got.dim() == 0 and got.dtype == torch.float32 and got.device.type == "cuda"
            exact, ref, hip = SO.shape64(y_hat, y, winlens), float(fixture[f"shape_{wname}_{iname}"]), float(got)
            print(f"shape {wname} {iname}: hip {hip:.9g} ref {ref:.9g} fp64 {exact:.9g}")
            if iname == "full":
                assert hip == 0.0
            elif not abs(hip - exact) <= 4 * abs(ref - exact) + 2.4e-7 * abs(exact):
                failures.append(f"{wname} {iname}: hip {hip} ref {ref} fp64 {exact}")
    assert not failures, "; ".join(failures)
    one = waveform_loss.WaveformShapeLoss(320)(a, b)
    assert torch.equal(one, waveform_loss.MultiWindowShapeLoss([320])(a, b))


def _eight(gpu, T=9600):
    y = torch.from_numpy(np.stack([MO._synth((1, T), 200 + i)[0] for i in range(8)])).to(gpu)
    y_hat = (y + 0.01 * torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(gpu)).contiguous()
    return y_hat, y


def test_grid_stride_stft_distance(gpu):
    """8 x 9600 at fft 256, hop 25: 3080 frame pairs over the 2048-workgroup cap, against eight one-signal calls folded into
    one accumulator."""
    from audiodec_amd import stft_loss
    y_hat, y = _eight(gpu)
    f = stft_loss.STFTLoss(256, 25, 256, device=gpu)
    assert f.num_frames(9600) * 8 == 3080

    def acc():
        return torch.zeros(3, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu)

    s_all, c_all = acc()
    f.fold(y_hat, y, s_all, c_all)
    s_one, c_one = acc()
    for i in range(8):
        f.fold(y_hat[i:i + 1], y[i:i + 1], s_one, c_one)
    assert int(c_all) == int(c_one) == 3080 * 129
    assert np.allclose(s_all.cpu().numpy(), s_one.cpu().numpy(), rtol=1e-12, atol=0)
    sc, mag = f(y_hat, y)
    s = s_all.cpu().numpy()
    assert float(sc) == pytest.approx(np.sqrt(s[0]) / np.sqrt(s[1]), rel=1e-6)
    assert float(mag) == pytest.approx(s[2] / int(c_all), rel=1e-6)


def test_grid_stride_mag_and_shape_distance(gpu):
    """Sizes over the workgroup caps of the two four-wave kernels (2048 x 1024 magnitudes; 2048 x 4 windows with a wave each at
    winlen 64; 2048 x 256 windows with a lane each at winlen 7), against the same sums composed from torch in f64."""
    from audiodec_amd import stft_loss, waveform_loss
    g = torch.Generator(device=gpu).manual_seed(11)
    xm = torch.rand(2, 4200, 257, device=gpu, generator=g) + 0.01
    ym = torch.rand(2, 4200, 257, device=gpu, generator=g) + 0.01
    assert xm.numel() > 2048 * 1024
    xd, yd = xm.double(), ym.double()
    sc = float(torch.linalg.norm((ym - xm).double()) / torch.linalg.norm(yd))         # d = y - x in f32, as the kernel takes it
    mag = float((yd.log() - xd.log()).abs().mean())
    assert float(stft_loss.SpectralConvergenceLoss()(xm, ym)) == pytest.approx(sc, rel=2e-7)
    # each f32 logf carries up to ~1 ulp of |log| <= 4.6, i.e. ~5e-7 absolute on a difference of mean 0.9, unbiased over 2e6 elements
    assert float(stft_loss.LogSTFTMagnitudeLoss()(xm, ym)) == pytest.approx(mag, rel=1e-6)
    y = torch.randn(256, 1, 48000, device=gpu, generator=g)
    y_hat = y + 0.1 * torch.randn(256, 1, 48000, device=gpu, generator=g)
    for w in (64, 7):
        assert 256 * (48000 // w) > 2048 * (4 if w >= 64 else 256)
        pa = torch.nn.functional.max_pool1d(y_hat.abs(), w).double()
        pb = torch.nn.functional.max_pool1d(y.abs(), w).double()
        exact = float((pa - pb).abs().mean())
        assert float(waveform_loss.WaveformShapeLoss(w)(y_hat, y)) == pytest.approx(exact, rel=2.4e-7)
    from audiodec_amd import native
    assert native.device_flags() == 0


def test_bitwise_reproducible(gpu):
    from audiodec_amd import stft_loss, waveform_loss
    loss = _loss("defaults", gpu)
    x, y = _pair("defaults", "synth3", gpu)
    a, b = loss(x, y), loss(x, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    y2 = y.reshape(-1, y.shape[-1])
    f = loss.stft_losses[0]
    m1, m2 = (stft_loss.stft(y2, f.fft_size, f.hop_size, f.win_length, f.window) for _ in range(2))
    assert torch.equal(m1, m2)
    xm = stft_loss.stft(x.reshape(-1, x.shape[-1]), f.fft_size, f.hop_size, f.win_length, f.window)
    assert torch.equal(stft_loss.SpectralConvergenceLoss()(xm, m1), stft_loss.SpectralConvergenceLoss()(xm, m1))
    assert torch.equal(stft_loss.LogSTFTMagnitudeLoss()(xm, m1), stft_loss.LogSTFTMagnitudeLoss()(xm, m1))
    shape = waveform_loss.MultiWindowShapeLoss()
    assert torch.equal(shape(x, y), shape(x, y))


def test_layouts_2d_and_3d(gpu):
    from audiodec_amd import waveform_loss
    loss = _loss("defaults", gpu)
    x, y = _pair("defaults", "synth3", gpu)                                # (3, 1, 9600)
    shape = waveform_loss.MultiWindowShapeLoss()
    for other in ((3, 9600), (1, 3, 9600)):
        l3, l2 = loss(x, y), loss(x.reshape(other), y.reshape(other))
        assert torch.equal(l3[0], l2[0]) and torch.equal(l3[1], l2[1])
        assert torch.equal(shape(x, y), shape(x.reshape(other), y.reshape(other)))
    f = loss.stft_losses[0]
    one = f(x, y)
    assert torch.equal(one[0], f(x.reshape(3, 9600), y.reshape(3, 9600))[0])


def test_nan_propagates_and_empty_is_nan(gpu):
    from audiodec_amd import native, stft_loss, waveform_loss
    loss = _loss("defaults", gpu)
    x, y = SO.inputs("defaults", "flat2")
    x = x.copy()
    x[0, 1000] = np.nan
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    sc, mag = loss(xt, yt)
    assert torch.isnan(sc) and torch.isnan(mag)
    f = loss.stft_losses[0]
    m = stft_loss.stft(xt, f.fft_size, f.hop_size, f.win_length, f.window)
    assert torch.isnan(m[0]).any() and torch.isfinite(m[1]).all()
    for w in (300, 7):                                                   # a wave per window, a lane per window
        assert torch.isnan(waveform_loss.WaveformShapeLoss(w)(xt, yt))
        assert torch.isnan(waveform_loss.WaveformShapeLoss(w)(yt, xt))
    # no signal: nothing is folded, the losses of an empty total are NaN
    sc, mag = loss(xt[:0], yt[:0])
    assert torch.isnan(sc) and torch.isnan(mag)
    assert torch.isnan(waveform_loss.MultiWindowShapeLoss()(xt[:0], yt[:0]))
    assert native.device_flags() == 0


def test_distances_over_batches(gpu):
    from audiodec_amd import stft_loss, waveform_loss
    y_hat, y = _eight(gpu)
    for pname in ("defaults", "edge"):
        d = stft_loss.STFTDistance(SO.PARAMS[pname], gpu)
        for i in range(4):
            d.update(y_hat[2 * i:2 * i + 2], y[2 * i:2 * i + 2])
        one = stft_loss.STFTDistance(SO.PARAMS[pname], gpu).update(y_hat, y)
        assert d.count() == one.count() == [8 * (1 + 9600 // h) * (n // 2 + 1) for n, h, _ in SO.resolutions(SO.PARAMS[pname])]
        assert d.value() == pytest.approx(one.value(), rel=1e-12)
        single = _loss(pname, gpu)(y_hat, y)
        assert d.value() == pytest.approx((float(single[0]), float(single[1])), rel=1e-6)
        d.reset()
        assert d.count() == [0] * 3 and all(np.isnan(v) for v in d.value())
    for winlen in ([300, 200, 100], [320], [7]):
        d = waveform_loss.ShapeDistance({"winlen": winlen}, gpu)
        for i in range(4):
            d.update(y_hat[2 * i:2 * i + 2], y[2 * i:2 * i + 2])
        one = waveform_loss.ShapeDistance({"winlen": winlen}, gpu).update(y_hat, y)
        assert d.count() == one.count() == [8 * (9600 // w) for w in winlen]
        assert d.value() == pytest.approx(one.value(), rel=1e-12)
        assert d.value() == pytest.approx(float(waveform_loss.MultiWindowShapeLoss(winlen)(y_hat, y)), rel=1e-6)
        d.reset()
        assert d.count() == [0] * len(winlen) and np.isnan(d.value())


def test_lazy_guard_result_as_input(gpu, ckpt_root):
    """decode's lazy-guard result gives the same values as a materialised copy of it."""
    from audiodec_amd import lazy_guard, stft_loss, synth, waveform_loss
    from audiodec_amd.audiodec import AudioDec, assign_model
    root = os.path.join(ckpt_root, "stft_lazy")
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
    loss, shape = _loss("defaults", gpu), waveform_loss.MultiWindowShapeLoss()
    with torch.no_grad():
        y = ad.decoder.decode(ad.rx_encoder.lookup(ad.tx_encoder.quantize(ad.tx_encoder.encode(x))))
        plain = lazy_guard.plain(y).clone()
        v_lazy, v_plain = loss(y, x), loss(plain, x)
        s_lazy, s_plain = shape(y, x), shape(plain, x)
    assert torch.equal(v_lazy[0], v_plain[0]) and torch.equal(v_lazy[1], v_plain[1]) and torch.equal(s_lazy, s_plain)
    d = stft_loss.STFTDistance(SO.PARAMS["defaults"], gpu).update(y, x)
    assert d.value() == pytest.approx((float(v_plain[0]), float(v_plain[1])), rel=1e-6)
    assert waveform_loss.ShapeDistance({"winlen": [300]}, gpu).update(y, x).value() == pytest.approx(
        float(waveform_loss.WaveformShapeLoss(300)(plain, x)), rel=1e-6)


def _loss_config(path, blocks=True):
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["use_stft_loss"] = False                                          # the flag of the driver is the opt-in, not this
    cfg["use_shape_loss"] = False
    if blocks:
        cfg["stft_loss_params"] = {k: v for k, v in SO.PARAMS["defaults"].items()}
        cfg["shape_loss_params"] = {"winlen": [300]}
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)


def test_testmain_stft_and_shape_distance(gpu, tmp_path):
    from audiodec_amd import offline, stft_loss, synth, waveform_loss
    from scipy.io import wavfile
    root = str(tmp_path)
    _, enc, dec = synth.write_model(root, "vctk_sym", 1337)
    cfg_path = os.path.join(os.path.dirname(enc), "config.yml")
    _loss_config(cfg_path, blocks=False)
    with pytest.raises(ValueError, match="stft_loss_params"):
        offline.TestMain(types.SimpleNamespace(encoder=enc, decoder=dec, stft_distance=True))
    with pytest.raises(ValueError, match="shape_loss_params"):
        offline.TestMain(types.SimpleNamespace(encoder=enc, decoder=dec, shape_distance=True))
    _loss_config(cfg_path)
    wavs = os.path.join(root, "wavs")
    os.makedirs(wavs)
    sig = {}
    for i, n in enumerate((4800, 7000)):
        pcm = np.clip(np.rint(MO._synth((n,), 400 + i) * 32767), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(wavs, f"utt{i}.wav"), 48000, pcm)
        sig[f"utt{i}"] = pcm.astype(np.float64) / 32768.0
    outs = {}
    only = offline.TestMain(types.SimpleNamespace(encoder=enc, decoder=dec, stft_distance=True))       # the flags are independent
    assert only.stft_loss is not None and only.shape_loss is None and only.mel_loss is None
    only = offline.TestMain(types.SimpleNamespace(encoder=enc, decoder=dec, shape_distance=True))
    assert only.stft_loss is None and only.shape_loss is not None
    for name, flags in (("none", {}), ("both", {"stft_distance": True, "shape_distance": True})):
        tm = offline.TestMain(types.SimpleNamespace(encoder=enc, decoder=dec, **flags))
        tm.dataset = offline.SingleDataset(files=wavs, query="*.wav", return_utt_id=True)
        tm.load_encoder()
        tm.load_decoder()
        out = os.path.join(root, f"out_{name}")
        tm.initial_folder("clean_test", out, "True")
        tm.run()
        outs[name] = (out, tm)
    wav_names = ["utt0_output.wav", "utt1_output.wav"]
    assert sorted(os.listdir(outs["none"][0])) == wav_names
    assert sorted(os.listdir(outs["both"][0])) == ["shape_distance.txt", "stft_distance.txt"] + wav_names
    none = outs["none"][1]
    assert none.mean_stft_distance is None and none.mean_shape_distance is None and none.mean_mel_distance is None
    out, tm = outs["both"]
    stft_vals = {line.split()[0]: [float(v) for v in line.split()[1:]]
                 for line in open(os.path.join(out, "stft_distance.txt")).read().split("\n") if line.strip()}
    shape_vals = {line.split()[0]: float(line.split()[1])
                  for line in open(os.path.join(out, "shape_distance.txt")).read().split("\n") if line.strip()}
    assert list(stft_vals) == ["utt0", "utt1", "mean"] and list(shape_vals) == ["utt0", "utt1", "mean"]
    assert stft_loss.from_config(tm.encoder_config) is None and waveform_loss.from_config(tm.encoder_config) is None
    loss = stft_loss.MultiResolutionSTFTLoss(**SO.PARAMS["defaults"], device=gpu)
    shape = waveform_loss.MultiWindowShapeLoss([300])
    d_stft, d_shape = {}, {}
    with torch.no_grad():
        for utt, x in sig.items():
            xt = torch.tensor(x, dtype=torch.float32)[None, None, :].to(gpu)
            y = tm.decode(tm.encode(x[:, None]))[..., :xt.shape[-1]]
            sc, mag = loss(y, xt)
            d_stft[utt] = [float(sc), float(mag)]
            d_shape[utt] = float(shape(y, xt))
    for utt in sig:
        assert stft_vals[utt] == pytest.approx(d_stft[utt], rel=1e-6)
        assert shape_vals[utt] == pytest.approx(d_shape[utt], rel=1e-6)
    mean_stft = np.mean(list(d_stft.values()), axis=0)
    assert stft_vals["mean"] == pytest.approx(list(mean_stft), rel=1e-6)
    assert shape_vals["mean"] == pytest.approx(np.mean(list(d_shape.values())), rel=1e-6)
    assert list(tm.mean_stft_distance) == pytest.approx(list(mean_stft), rel=1e-6)
    assert tm.mean_shape_distance == pytest.approx(np.mean(list(d_shape.values())), rel=1e-6)
