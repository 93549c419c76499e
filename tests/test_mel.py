"""CPU: the mel-spectrogram loss's host side (audiodec_amd.mel) and what tests/golden/mel.npz means.

  * the package's filter bank equals the fixture's melmat (the reference's, made by make_mel_golden.py) and has the Slaney
    mel scale's properties; its sparse form holds the same weights;
  * the fp64 restatement (mel_oracle) reproduces the reference's float32 log-mels and losses within float32 round-off;
  * frame counts, and every argument error, raised before any device use;
  * the adk_logmel / adk_mel_distance / adk_mel_workspace_bytes argument checks, which run on the host before any HIP call.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import mel_oracle as MO

ADK_ERR_ARG = -1


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mel.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


@pytest.mark.parametrize("pname", list(MO.PARAMS))
def test_filterbank_equals_fixture(fixture, pname):
    from audiodec_amd import mel
    p = MO.params(pname)
    for r, (n_fft, _, _) in enumerate(MO.resolutions(p)):
        mm = mel.mel_filterbank(p["fs"], n_fft, p["num_mels"], p["fmin"], p["fmax"])
        assert mm.dtype == np.float32 and mm.shape == (p["num_mels"], n_fft // 2 + 1)
        assert np.array_equal(mm, fixture[f"{pname}_melmat{r}"]), f"{pname} resolution {r}"


def test_slaney_mel_scale():
    from audiodec_amd import mel
    assert mel.hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12)
    assert mel.hz_to_mel(500.0) == pytest.approx(7.5, abs=1e-12)                     # linear below 1 kHz: 200/3 Hz per mel
    step = math.log(6.4) / 27
    assert mel.hz_to_mel(1000.0 * math.exp(step * 10)) == pytest.approx(25.0, abs=1e-9)  # log step ln(6.4)/27 above
    f = np.array([0.0, 300.0, 999.0, 1000.0, 4000.0, 24000.0])
    assert np.allclose(mel.mel_to_hz(mel.hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("pname", ["vctk", "libritts", "log2"])
def test_filters_integrate_to_one(pname):
    """norm='slaney': each triangle has area 1 over Hz (checked where a filter spans enough bins to integrate it)."""
    from audiodec_amd import mel
    p = MO.params(pname)
    n_fft = p["fft_sizes"][0]
    mm = mel.mel_filterbank(p["fs"], n_fft, p["num_mels"], p["fmin"], p["fmax"]).astype(np.float64)
    df = p["fs"] / n_fft
    wide = (mm > 0).sum(1) >= 8
    assert wide.sum() >= 20
    assert np.allclose(mm[wide].sum(1) * df, 1.0, atol=0.03)
    assert ((mm > 0).sum(1) > 0).all(), "an empty filter"


def test_sparse_filters_hold_the_weights():
    from audiodec_amd import mel
    p = MO.params("vctk")
    mm = mel.mel_filterbank(p["fs"], 2048, 80, 0, 24000)
    rng, w = mel.sparse_filters(mm)
    dense = np.zeros_like(mm)
    for m, (first, count, off) in enumerate(rng):
        dense[m, first:first + count] = w[off:off + count]
    assert np.array_equal(dense, mm)
    assert rng[:, 1].max() == 102                          # the widest filter at 48 kHz / 2048 / 80 mels
    assert (mm > 0).sum(0).max() <= 2                      # no bin in more than two filters
    assert int(w.size) == int(rng[-1, 1] + rng[-1, 2])


def mel_error(logmel, exact, log_base):
    """max |mel - mel_fp64| relative to the largest mel of its frame: the scale of float32 FFT round-off.  (The log-mels
    themselves are compared in test_gpu_mel against 4x the reference's own error: bands whose energy is at the round-off
    floor -- the synthetic audio has almost none below 100 Hz -- carry log errors of 1e-2 in the reference too.)"""
    b = np.e if log_base is None else log_base
    m, mo = np.power(b, np.asarray(logmel, np.float64)), np.power(b, exact)
    return float(np.max(np.abs(m - mo) / mo.max(axis=1, keepdims=True)))


@pytest.mark.parametrize("pname", list(MO.PARAMS))
def test_fp64_oracle_reproduces_fixture(fixture, pname):
    p = MO.params(pname)
    res = MO.resolutions(p)
    melmats = [fixture[f"{pname}_melmat{r}"] for r in range(len(res))]
    for iname in MO.INPUTS:
        y_hat, y = MO.inputs(pname, iname)
        if (pname, iname) in MO.LOGMEL_CASES:
            for r, ((n_fft, hop, wl), mm) in enumerate(zip(res, melmats)):
                ref = fixture[f"{pname}_{iname}_logmel{r}"]
                o = MO.logmel64(y, p["fs"], n_fft, hop, wl, mm, p["eps"], p["log_base"])
                assert ref.shape == o.shape == (int(np.prod(y.shape[:-1])), p["num_mels"], 1 + y.shape[-1] // hop)
                assert mel_error(ref, o, p["log_base"]) < 2e-6, f"{pname} {iname} r{r}"
        # the L1 of log-mels weighs the round-off-floor bands fully: the reference's float32 loss is within 0.3 % of fp64 here
        ref_loss = float(fixture[f"{pname}_{iname}_loss"])
        assert MO.loss64(y_hat, y, p, melmats) == pytest.approx(ref_loss, rel=5e-3, abs=1e-9), f"{pname} {iname}"


def test_silence_logmel_value(fixture):
    """Silence: every bin clamps to sqrt(1e-10) = 1e-5, so each filter gives log(1e-5 * sum of its weights), about -14.67 at
    48 kHz / 2048 -- the second clamp is never reached."""
    mm = fixture["vctk_melmat0"].astype(np.float64)
    expect = np.log(1e-5 * mm.sum(1))
    o = MO.logmel64(np.zeros((1, 4800)), 48000, 2048, 300, 2048, mm)
    assert np.allclose(o[0], expect[:, None], atol=1e-12)
    assert np.all(np.abs(expect - (-14.67)) < 0.05)


def test_frame_counts_and_errors_before_device_use():
    from audiodec_amd import mel
    assert mel.num_frames(9600, 300) == 33 and mel.num_frames(7777, 300) == 26 and mel.num_frames(1025, 300) == 4
    m = mel.MelSpectrogram(fs=48000, fft_size=2048, hop_size=300, win_length=None, fmin=0, fmax=24000, log_base=None)
    assert m.win_length == 2048 and m.num_frames(4500) == 16 and m._dev is None
    with pytest.raises(ValueError, match="reflect padding"):
        m(torch.zeros(1, 1024))
    with pytest.raises(ValueError, match="reflect padding"):
        mel.MultiMelSpectrogramLoss(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048])(torch.zeros(2, 1000),
                                                                                                      torch.zeros(2, 1000))
    for bad in (1000, 128, 8192):
        with pytest.raises(NotImplementedError, match="fft_size"):
            mel.MelSpectrogram(fft_size=bad, win_length=100)
    with pytest.raises(NotImplementedError, match="window"):
        mel.MelSpectrogram(window="hamming_window")
    with pytest.raises(ValueError, match="log_base: 3.0 is not supported"):
        mel.MelSpectrogram(log_base=3.0)
    with pytest.raises(ValueError, match="log_base"):
        mel.MultiMelSpectrogramLoss(log_base=np.e)
    m = mel.MelSpectrogram(center=False, normalized=True, onesided=False)        # accepted, stored, ignored: as the reference
    assert (m.center, m.normalized, m.onesided) == (False, True, False)
    with pytest.raises(ValueError, match="same shape"):
        mel.MultiMelSpectrogramLoss()(torch.zeros(1, 3000), torch.zeros(1, 3001))


def test_grad_is_refused():
    from audiodec_amd import mel
    x = torch.zeros(1, 4800, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        mel.MelSpectrogram()(x)
    with pytest.raises(NotImplementedError, match="forward only"):
        mel.MultiMelSpectrogramLoss()(x, torch.zeros(1, 4800))


def test_from_config():
    from audiodec_amd import mel
    assert mel.from_config({"use_mel_loss": False, "mel_loss_params": {}}) is None
    assert mel.from_config({}) is None
    cfg = {"use_mel_loss": True, "mel_loss_params": dict(MO.PARAMS["denoise"])}
    loss = mel.from_config(cfg)
    assert isinstance(loss, mel.MultiMelSpectrogramLoss) and len(loss.mel_transfers) == 1
    assert loss.mel_transfers[0].win_length == 2048 and loss.mel_transfers[0].log_base is None


def test_mel_symbols_are_bound(lib):
    from audiodec_amd import native
    for name in ("adk_logmel", "adk_mel_distance", "adk_mel_workspace_bytes"):
        assert name in native.SYMBOLS and getattr(lib, name) is not None


def test_argument_validation_without_device(lib):
    from audiodec_amd import mel
    mm = mel.mel_filterbank(48000, 2048, 80, 0, 24000)
    rng, w = mel.sparse_filters(mm)
    win = np.hanning(2048).astype(np.float32)
    # host arrays stand in for device pointers: every call below must fail (or finish) before touching them
    R, W, Wn = rng.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)
    acc = np.zeros(2, np.float64)
    S, N = acc[:1].ctypes.data_as(C.c_void_p), acc[1:].ctypes.data_as(C.c_void_p)
    dummy = C.c_void_p(16)

    def logmel(n=2, T=4800, n_fft=2048, hop=300, wl=2048, nm=80, lb=0, out=dummy, x=dummy, win=Wn):
        return lib.adk_logmel(x, n, T, n_fft, hop, win, wl, R, W, int(w.size), nm, lb, C.c_float(1e-10), out, None)

    def dist(n=2, T=4800, n_fft=2048, s=S, c=N, ws=dummy, loss=None):
        return lib.adk_mel_distance(dummy, dummy, n, T, n_fft, 300, Wn, 2048, R, W, int(w.size), 80, 0, C.c_float(1e-10),
                                    s, c, ws, loss, None)

    for bad in (1000, 128, 8192, 0):
        assert logmel(n_fft=bad) == ADK_ERR_ARG and b"power of two" in lib.adk_last_error()
    assert logmel(T=1024) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
    assert logmel(hop=0) == ADK_ERR_ARG
    assert logmel(wl=4096) == ADK_ERR_ARG and logmel(wl=0) == ADK_ERR_ARG
    assert logmel(nm=0) == ADK_ERR_ARG and logmel(nm=257) == ADK_ERR_ARG
    assert logmel(lb=3) == ADK_ERR_ARG and b"log_base" in lib.adk_last_error()
    assert logmel(out=None) == ADK_ERR_ARG and logmel(win=None) == ADK_ERR_ARG
    assert logmel(out=C.c_void_p(18)) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error()
    assert logmel(n=-1) == ADK_ERR_ARG
    assert logmel(n=0, x=None, out=None) == 0                                  # nothing to do: no launch
    assert dist(s=None) == ADK_ERR_ARG and b"accumulator" in lib.adk_last_error()
    assert dist(ws=None) == ADK_ERR_ARG
    assert dist(s=C.c_void_p(S.value + 4)) == ADK_ERR_ARG and b"8-byte" in lib.adk_last_error()
    assert dist(T=1000) == ADK_ERR_ARG
    assert dist(n=0, ws=None) == 0                                             # nothing folded, no loss asked for: no launch
    assert lib.adk_mel_workspace_bytes(0, 4800, 2048, 300) == 0
    assert lib.adk_mel_workspace_bytes(16, 9600, 2048, 300) == 16 * 33 * 8
    assert lib.adk_mel_workspace_bytes(256, 48000, 2048, 300) == 2048 * 8        # capped at 2048 workgroups
    assert lib.adk_mel_workspace_bytes(1, 4800, 2048, 0) == ADK_ERR_ARG
    assert acc.tolist() == [0.0, 0.0]
