"""CPU: the host side of the STFT and waveform-shape losses (audiodec_amd.stft_loss, audiodec_amd.waveform_loss) and what
tests/golden/stft_loss.npz means.

  * the fp64 restatement (stft_oracle) agrees with the reference's float32 values within float32 round-off:
    rel <= 1e-5 for both STFT terms and the shape loss, <= 1e-3 for the STFT terms of "tone", whose leakage bins sit next to
    the 1e-7 clamp (the reference was probed at 5e-9..3.3e-6 for sc, 7e-9..1.6e-6 / 1.3e-4..1.7e-4 on tone for mag, <= 1e-7
    for the shape loss);
  * frame counts, the placement of the window, the T // winlen rule;
  * every argument error of the Python classes, raised before any device use; from_config;
  * the adk_stft_* / adk_mag_distance / adk_shape_* argument checks, which run on the host before any HIP call;
  * every declaration of the header's new block is exported and bound.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stft_oracle as SO

ADK_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("adk_stft_workspace_bytes", "adk_stft_mag", "adk_stft_distance", "adk_mag_distance_workspace_bytes",
               "adk_mag_distance", "adk_shape_workspace_bytes", "adk_shape_distance")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "stft_loss.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def rel(v, exact):
    return abs(float(v) - exact) / abs(exact) if exact != 0 else abs(float(v))


@pytest.mark.parametrize("pname", list(SO.PARAMS))
def test_fp64_oracle_agrees_with_fixture_losses(fixture, pname):
    for iname in SO.INPUTS:
        sc, mag = SO.exact_loss(pname, iname)
        bound = 1e-3 if iname == "tone" else 1e-5
        e_sc, e_mag = rel(fixture[f"{pname}_{iname}_sc"], sc), rel(fixture[f"{pname}_{iname}_mag"], mag)
        print(f"{pname} {iname}: e(ref sc) {e_sc:.3g}  e(ref mag) {e_mag:.3g}")
        assert e_sc <= bound, f"{pname} {iname}: sc ref {fixture[f'{pname}_{iname}_sc']} fp64 {sc}"
        assert e_mag <= bound, f"{pname} {iname}: mag ref {fixture[f'{pname}_{iname}_mag']} fp64 {mag}"


@pytest.mark.parametrize("case", SO.MAG_CASES, ids=lambda c: "-".join(c))
def test_fp64_oracle_agrees_with_fixture_magnitudes(fixture, case):
    pname, iname = case
    p = SO.PARAMS[pname]
    _, y = SO.inputs(pname, iname)
    n = int(np.prod(y.shape[:-1]))
    for r, (n_fft, hop, wl) in enumerate(SO.resolutions(p)):
        ref = fixture[f"{pname}_{iname}_ymag{r}"]
        o = SO.mag64(y, n_fft, hop, wl, SO.window_f32(p["window"], wl))
        assert ref.dtype == np.float32 and ref.shape == o.shape == (n, 1 + y.shape[-1] // hop, n_fft // 2 + 1)
        # float32 FFT round-off, relative to the largest magnitude of the frame (the scale docs/design/mel.md uses)
        assert np.max(np.abs(ref - o) / o.max(axis=-1, keepdims=True)) < 2e-6, f"{pname} {iname} r{r}"


def test_fp64_oracle_agrees_with_fixture_shape(fixture):
    for wname in SO.SHAPE_WINLENS:
        for iname in SO.SHAPE_INPUTS:
            y_hat, y = SO.inputs("defaults", iname)
            exact = SO.shape64(y_hat, y, SO.shape_winlens(wname, y.shape[-1]))
            ref = float(fixture[f"shape_{wname}_{iname}"])
            if iname == "full":
                assert exact == 0.0 and ref == 0.0
            else:
                assert rel(ref, exact) <= 1e-5, f"{wname} {iname}: ref {ref} fp64 {exact}"


def test_frames_window_placement_and_windows():
    from audiodec_amd import stft_loss, waveform_loss
    f = stft_loss.STFTLoss(512, 100, 511)
    assert f.num_frames(7777) == 78 and f.num_frames(257) == 3 and SO.num_frames(7777, 100) == 78
    assert stft_loss.STFTLoss(1024, 120, 600).num_frames(9600) == 81
    assert SO.left_pad(512, 511) == 0 and SO.left_pad(1024, 600) == 212 and SO.left_pad(256, 200) == 28
    # an impulse at sample t (away from the reflected ends) shows the window value that multiplies it: frame f starts
    # n_fft // 2 - f hop before the signal, so the sample meets window value t + n_fft // 2 - f hop - left_pad and gives a
    # flat spectrum of that height; in frame 4 it falls into the zeros left of the window
    n_fft, hop, wl = 256, 64, 200
    win = SO.window_f32("hann_window", wl)
    x = np.zeros((1, 300))
    x[0, 150] = 1.0
    m = SO.mag64(x, n_fft, hop, wl, win, eps=0.0)
    assert m.shape == (1, 5, 129)
    assert np.allclose(m[0, 1], win[150 + 128 - 64 - 28], atol=1e-12) and np.allclose(m[0, 2], win[150 + 128 - 128 - 28], atol=1e-12)
    assert np.allclose(m[0, 0], 0, atol=1e-12) and np.allclose(m[0, 4], 0, atol=1e-12)
    # the same through torch.stft, which the restatement stands for
    t = torch.stft(torch.from_numpy(x), n_fft, hop, wl, torch.from_numpy(win).double(), return_complex=True).abs().transpose(2, 1)
    assert np.allclose(t.numpy(), m, atol=1e-12)
    assert waveform_loss.num_windows(7777, 300) == 25 and waveform_loss.num_windows(300, 300) == 1
    assert waveform_loss.num_windows(7777, 7) == 1111
    # the tail is dropped: changing it changes nothing
    a, b = np.zeros((1, 650)), np.zeros((1, 650))
    a[0, 100], a[0, 640] = 0.5, 0.9
    assert SO.shape64(a, b, [300]) == 0.25
    ref = torch.nn.functional.l1_loss(torch.nn.functional.max_pool1d(torch.from_numpy(a).abs()[None], 300),
                                      torch.nn.functional.max_pool1d(torch.from_numpy(b).abs()[None], 300))
    assert float(ref) == 0.25


def test_errors_before_device_use():
    from audiodec_amd import stft_loss, waveform_loss
    for bad in (1000, 128, 8192):
        with pytest.raises(NotImplementedError, match="fft_size"):
            stft_loss.STFTLoss(bad, 100, 100)
        with pytest.raises(NotImplementedError, match="fft_size"):
            stft_loss.MultiResolutionSTFTLoss([1024, bad], [120, 100], [600, 100])
        with pytest.raises(NotImplementedError, match="fft_size"):
            stft_loss.stft(torch.zeros(1, 9000), bad, 100, 100, torch.ones(100))
    with pytest.raises(ValueError, match="win_length"):
        stft_loss.STFTLoss(512, 100, 513)
    with pytest.raises(ValueError, match="hop_size"):
        stft_loss.STFTLoss(512, 0, 512)
    with pytest.raises(AttributeError):
        stft_loss.STFTLoss(window="no_such_window")
    loss = stft_loss.MultiResolutionSTFTLoss()
    assert [(f.fft_size, f.hop_size, f.win_length) for f in loss.stft_losses] == [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]
    assert loss.device is None and torch.equal(loss.stft_losses[0].window, torch.hann_window(600))
    assert torch.equal(stft_loss.STFTLoss(512, 128, 400, "hamming_window").window, torch.hamming_window(400))
    f = stft_loss.STFTLoss()
    assert (f.fft_size, f.hop_size, f.win_length) == (1024, 120, 600)
    with pytest.raises(ValueError, match="reflect padding"):
        loss(torch.zeros(2, 1024), torch.zeros(2, 1024))
    with pytest.raises(ValueError, match="reflect padding"):
        f(torch.zeros(2, 512), torch.zeros(2, 512))
    with pytest.raises(ValueError, match="reflect padding"):
        stft_loss.stft(torch.zeros(1, 128), 256, 64, 200, torch.ones(200))
    with pytest.raises(ValueError, match="same shape"):
        loss(torch.zeros(1, 3000), torch.zeros(1, 3001))
    with pytest.raises(ValueError, match="window"):
        stft_loss.stft(torch.zeros(1, 3000), 256, 64, 200, torch.ones(199))
    with pytest.raises(ValueError, match="shorter than winlen"):
        waveform_loss.WaveformShapeLoss(300)(torch.zeros(1, 1, 299), torch.zeros(1, 1, 299))
    with pytest.raises(ValueError, match="shorter than winlen"):
        waveform_loss.MultiWindowShapeLoss()(torch.zeros(2, 1, 250), torch.zeros(2, 1, 250))
    with pytest.raises(ValueError, match="winlen"):
        waveform_loss.WaveformShapeLoss(0)
    with pytest.raises(ValueError, match="same shape"):
        waveform_loss.MultiWindowShapeLoss()(torch.zeros(1, 1, 400), torch.zeros(1, 1, 401))
    assert [f.winlen for f in waveform_loss.MultiWindowShapeLoss().shape_losses] == [300, 200, 100]


def test_grad_is_refused():
    from audiodec_amd import stft_loss, waveform_loss
    x = torch.zeros(1, 4800, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        stft_loss.MultiResolutionSTFTLoss()(x, torch.zeros(1, 4800))
    with pytest.raises(NotImplementedError, match="forward only"):
        stft_loss.stft(x, 256, 64, 200, torch.ones(200))
    with pytest.raises(NotImplementedError, match="forward only"):
        stft_loss.SpectralConvergenceLoss()(x, torch.zeros(1, 4800))
    with pytest.raises(NotImplementedError, match="forward only"):
        waveform_loss.MultiWindowShapeLoss()(x, torch.zeros(1, 4800))


def test_from_config():
    from audiodec_amd import stft_loss, waveform_loss
    cfg = {"use_stft_loss": False, "stft_loss_params": dict(SO.PARAMS["defaults"]), "use_shape_loss": False,
           "shape_loss_params": {"winlen": [300]}}
    assert stft_loss.from_config(cfg) is None and waveform_loss.from_config(cfg) is None
    assert stft_loss.from_config({}) is None and waveform_loss.from_config({}) is None
    cfg["use_stft_loss"] = cfg["use_shape_loss"] = True
    loss = stft_loss.from_config(cfg)
    assert isinstance(loss, stft_loss.MultiResolutionSTFTLoss) and len(loss.stft_losses) == 3
    shape = waveform_loss.from_config(cfg)
    assert isinstance(shape, waveform_loss.MultiWindowShapeLoss) and [f.winlen for f in shape.shape_losses] == [300]


def test_new_declarations_are_exported_and_bound(lib):
    from audiodec_amd import native
    with open(os.path.join(ROOT, "include", "audiodec_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(adk_(?:stft|mag_distance|shape)\w*)\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert lib.adk_abi_version() == 14


def test_argument_validation_without_device(lib):
    win = np.hanning(600).astype(np.float32)
    # host arrays stand in for device pointers: every call below must fail (or finish) before touching them
    Wn = win.ctypes.data_as(C.c_void_p)
    acc = np.zeros(4, np.float64)
    S, N = acc[:3].ctypes.data_as(C.c_void_p), acc[3:].ctypes.data_as(C.c_void_p)
    dummy = C.c_void_p(16)
    eps = C.c_float(1e-7)

    def mag(n=2, T=4800, n_fft=1024, hop=120, wl=600, out=dummy, x=dummy, win=Wn):
        return lib.adk_stft_mag(x, n, T, n_fft, hop, win, wl, eps, out, None)

    def dist(n=2, T=4800, n_fft=1024, hop=120, wl=600, x=dummy, y=dummy, s=S, c=N, ws=dummy, sc=None, mg=None, win=Wn):
        return lib.adk_stft_distance(x, y, n, T, n_fft, hop, win, wl, eps, s, c, ws, sc, mg, None)

    def magd(n=1000, x=dummy, y=dummy, s=S, c=N, ws=dummy, sc=None, mg=None):
        return lib.adk_mag_distance(x, y, n, s, c, ws, sc, mg, None)

    def shape(n=2, T=4800, wl=300, a=dummy, b=dummy, s=S, c=N, ws=dummy, loss=None):
        return lib.adk_shape_distance(a, b, n, T, wl, s, c, ws, loss, None)

    for fn in (mag, dist):
        for bad in (1000, 128, 8192, 0):
            assert fn(n_fft=bad) == ADK_ERR_ARG and b"power of two" in lib.adk_last_error()
        assert fn(T=512) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
        assert fn(hop=0) == ADK_ERR_ARG and b"hop" in lib.adk_last_error()
        assert fn(wl=1025) == ADK_ERR_ARG and fn(wl=0) == ADK_ERR_ARG and b"win_length" in lib.adk_last_error()
        assert fn(n=-1) == ADK_ERR_ARG
        assert fn(win=None) == ADK_ERR_ARG and b"null" in lib.adk_last_error()
        assert fn(win=C.c_void_p(Wn.value + 2)) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error()
        assert fn(x=None) == ADK_ERR_ARG and b"null" in lib.adk_last_error()
        assert fn(x=C.c_void_p(18)) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error()
    assert mag(out=None) == ADK_ERR_ARG and mag(out=C.c_void_p(18)) == ADK_ERR_ARG
    assert mag(n=0, x=None, out=None) == 0                                     # nothing to do: no launch
    assert dist(y=None) == ADK_ERR_ARG
    for fn in (dist, magd, shape):
        assert fn(s=None) == ADK_ERR_ARG and b"accumulator" in lib.adk_last_error()
        assert fn(c=None) == ADK_ERR_ARG
        assert fn(ws=None) == ADK_ERR_ARG and b"null" in lib.adk_last_error()
        assert fn(s=C.c_void_p(S.value + 4)) == ADK_ERR_ARG and b"8-byte" in lib.adk_last_error()
        assert fn(ws=C.c_void_p(20)) == ADK_ERR_ARG and b"8-byte" in lib.adk_last_error()
        assert fn(n=0, ws=None) == 0                                           # nothing folded, no result asked for: no launch
    assert dist(sc=C.c_void_p(18)) == ADK_ERR_ARG and dist(mg=C.c_void_p(18)) == ADK_ERR_ARG
    assert magd(mg=C.c_void_p(18)) == ADK_ERR_ARG and shape(loss=C.c_void_p(18)) == ADK_ERR_ARG
    assert magd(n=-1) == ADK_ERR_ARG and magd(x=None) == ADK_ERR_ARG and magd(y=C.c_void_p(18)) == ADK_ERR_ARG
    assert shape(wl=0) == ADK_ERR_ARG and b"winlen" in lib.adk_last_error()
    assert shape(T=299) == ADK_ERR_ARG and b"winlen" in lib.adk_last_error()
    assert shape(n=-1) == ADK_ERR_ARG and shape(a=None) == ADK_ERR_ARG and shape(b=C.c_void_p(18)) == ADK_ERR_ARG
    # the slabs: three (one) f64 per workgroup, one workgroup per frame (per 1024 elements; per 4 or 256 windows), at most 2048
    assert lib.adk_stft_workspace_bytes(0, 4800, 1024, 120) == 0
    assert lib.adk_stft_workspace_bytes(16, 9600, 1024, 120) == 16 * 81 * 24
    assert lib.adk_stft_workspace_bytes(8, 9600, 256, 25) == 2048 * 24          # 3080 frames, capped
    assert lib.adk_stft_workspace_bytes(1, 4800, 1024, 0) == ADK_ERR_ARG
    assert lib.adk_mag_distance_workspace_bytes(0) == 0 and lib.adk_mag_distance_workspace_bytes(-1) == ADK_ERR_ARG
    assert lib.adk_mag_distance_workspace_bytes(1025) == 2 * 24
    assert lib.adk_mag_distance_workspace_bytes(1 << 40) == 2048 * 24
    assert lib.adk_shape_workspace_bytes(0, 4800, 300) == 0
    assert lib.adk_shape_workspace_bytes(2, 4800, 300) == 8 * 8                 # 32 windows, a wave each, 4 waves per workgroup
    assert lib.adk_shape_workspace_bytes(2, 4800, 64) == 38 * 8                 # 150 windows, a wave each
    assert lib.adk_shape_workspace_bytes(2, 4800, 63) == 1 * 8                  # 152 windows, a lane each
    assert lib.adk_shape_workspace_bytes(256, 48000, 7) == 2048 * 8
    assert lib.adk_shape_workspace_bytes(2, 299, 300) == ADK_ERR_ARG and lib.adk_shape_workspace_bytes(2, 300, 0) == ADK_ERR_ARG
    assert acc.tolist() == [0.0] * 4
