"""CPU: the mel-spectrogram loss's backward -- host side, and what tests/golden/mel_grad.npz means.

  * the fp64 restatement (mel_grad_oracle) reproduces the reference's float32 autograd gradients stored in the fixture;
  * the transposed sparse filter table holds melmat.T;
  * `differentiable` defaults to False and the refusal of grad inputs stays; y may never require grad;
  * the adk_logmel_vjp / adk_mel_distance_grad / adk_mel_grad_workspace_bytes bindings and their argument checks, which run on the
    host before any HIP call.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mel_grad_oracle as GO
import mel_oracle as MO

ADK_ERR_ARG = -1
STORED = [c for c in GO.CASES if GO.stored(c[1])]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mel_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def test_fixture_covers_every_case(fixture):
    assert len(GO.CASES) == 12 and len(STORED) == 10
    for pname, shape in GO.CASES:
        K, R = GO.key(pname, shape), len(GO.params(pname)["fft_sizes"])
        assert 0 < float(fixture[f"{K}_relerr32_loss"]) < 1e-5 and int(fixture[f"{K}_signdiff"]) == 0
        for r in range(R):
            assert 0 < float(fixture[f"{K}_relerr32_vjp{r}"]) < 1e-5
            assert (f"{K}_vjp{r}" in fixture.files) == GO.stored(shape)
        assert (f"{K}_lossgrad" in fixture.files) == GO.stored(shape)


@pytest.mark.parametrize("pname,shape", STORED, ids=[GO.key(*c) for c in STORED])
def test_fp64_oracle_reproduces_reference_gradients(fixture, pname, shape):
    p, K = GO.params(pname), GO.key(pname, shape)
    mms = GO.melmats(p)
    y_hat, y = GO.inputs(shape)
    n = int(np.prod(shape[:-1]))
    ref = fixture[f"{K}_lossgrad"]
    g = GO.loss_grad64(y_hat, y, p, mms)
    assert g.shape == ref.shape == (n, shape[-1])
    err = GO.rel_l2(ref, g)
    print(f"{K}: loss gradient, reference f32 against the oracle: {err:.3g}")
    assert err <= 1e-5
    for r, (n_fft, hop, wl) in enumerate(MO.resolutions(p)):
        v = GO.vjp64(y_hat, GO.upstream(pname, shape, r, p), n_fft, hop, wl, mms[r], p["eps"], p["log_base"])
        err = GO.rel_l2(fixture[f"{K}_vjp{r}"], v)
        print(f"{K} r{r}: VJP, reference f32 against the oracle: {err:.3g}")
        assert err <= 1e-5


def test_oracle_sign_override_and_coverage():
    p = GO.params("gap")
    mms = GO.melmats(p)
    y_hat, y = GO.inputs((2, 1, 2000))
    own = [s for s, _ in GO.signs64(y_hat, y, p, mms)]
    g = GO.loss_grad64(y_hat, y, p, mms)
    assert np.array_equal(GO.loss_grad64(y_hat, y, p, mms, signs=own), g)
    assert np.array_equal(GO.loss_grad64(y_hat, y, p, mms, signs=[-s for s in own]), -g)
    cov = GO.coverage(2000, 256, 300, 256)
    assert int((cov == 0).sum()) * 2 == 684                                 # what the reference's gradient has
    assert np.array_equal(g == 0, np.broadcast_to(cov == 0, g.shape))


@pytest.mark.parametrize("pname", ["vctk", "defaults", "log2", "small", "big", "gap"])
def test_transposed_filters_hold_melmat_t(pname):
    from audiodec_amd import mel
    p = GO.params(pname)
    for mm in GO.melmats(p):
        rng, w = mel.transposed_filters(mm)
        assert rng.dtype == np.int32 and w.dtype == np.float32 and rng.shape == (mm.shape[1], 3)
        dense = np.zeros_like(mm.T)
        for k, (first, count, off) in enumerate(rng):
            dense[k, first:first + count] = w[off:off + count]
        assert np.array_equal(dense, mm.T)
        assert int(w.size) == max(int(rng[:, 1].sum()), 1)
        f = mel.MelSpectrogram(fs=p["fs"], fft_size=mm.shape[1] * 2 - 2, hop_size=64, num_mels=p["num_mels"], fmin=p["fmin"],
                               fmax=p["fmax"], log_base=p["log_base"])
        assert np.array_equal(f._trange, rng) and np.array_equal(f._tweights, w)
    assert GO.params("big")["num_mels"] > 64                                   # more than one filter per lane


def test_differentiable_defaults_to_false_and_refusal_stays():
    from audiodec_amd import mel
    assert mel.MelSpectrogram().differentiable is False
    loss = mel.MultiMelSpectrogramLoss()
    assert loss.differentiable is False and not any(f.differentiable for f in loss.mel_transfers)
    cfg = {"use_mel_loss": True, "mel_loss_params": dict(MO.PARAMS["vctk"])}
    assert mel.from_config(cfg).differentiable is False
    d = mel.from_config(cfg, differentiable=True)
    assert d.differentiable is True and all(f.differentiable for f in d.mel_transfers)
    assert mel.from_config({}, differentiable=True) is None
    x = torch.zeros(1, 4800, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        mel.MelSpectrogram()(x)
    with pytest.raises(NotImplementedError, match="forward only"):
        loss(x, torch.zeros(1, 4800))
    with pytest.raises(NotImplementedError, match="forward only"):
        loss(torch.zeros(1, 4800), x)


def test_target_requiring_grad_is_refused():
    from audiodec_amd import mel
    loss = mel.MultiMelSpectrogramLoss(differentiable=True)
    y = torch.zeros(1, 4800, requires_grad=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        loss(torch.zeros(1, 4800), y)
    with pytest.raises(NotImplementedError, match="forward only"):
        loss(torch.zeros(1, 4800, requires_grad=True), y)
    with pytest.raises(ValueError, match="reflect padding"):                    # argument errors still come first
        loss(torch.zeros(1, 500, requires_grad=True), torch.zeros(1, 500))
    with pytest.raises(ValueError, match="reflect padding"):
        mel.MelSpectrogram(differentiable=True)(torch.zeros(1, 500, requires_grad=True))


def test_grad_symbols_are_bound(lib):
    from audiodec_amd import native
    for name in ("adk_logmel_vjp", "adk_mel_distance_grad", "adk_mel_grad_workspace_bytes"):
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    from audiodec_amd import mel
    mm = mel.mel_filterbank(48000, 2048, 80, 0, 24000)
    rng, w = mel.sparse_filters(mm)
    trng, tw = mel.transposed_filters(mm)
    win = np.hanning(2048).astype(np.float32)
    # host arrays stand in for device pointers: every call below must fail (or finish) before touching them
    R, W, Wn = rng.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)
    TR, TW = trng.ctypes.data_as(C.c_void_p), tw.ctypes.data_as(C.c_void_p)
    dummy = C.c_void_p(16)

    def vjp(n=2, T=4800, n_fft=2048, hop=300, x=dummy, g=dummy, ws=dummy, out=dummy, tr=TR, ntw=int(tw.size), win=Wn):
        return lib.adk_logmel_vjp(x, g, n, T, n_fft, hop, win, 2048, R, W, int(w.size), 80, 0, C.c_float(1e-10), tr, TW, ntw,
                                  ws, out, None)

    def dgrad(n=2, T=4800, n_fft=2048, a=dummy, b=dummy, up=dummy, ws=dummy, out=dummy, nm=80, lb=0):
        return lib.adk_mel_distance_grad(a, b, n, T, n_fft, 300, Wn, 2048, R, W, int(w.size), nm, lb, C.c_float(1e-10), TR, TW,
                                         int(tw.size), 1.0 / 1000, up, ws, out, None)

    for bad in (1000, 128, 8192, 0):
        assert vjp(n_fft=bad) == ADK_ERR_ARG and b"power of two" in lib.adk_last_error()
        assert dgrad(n_fft=bad) == ADK_ERR_ARG and b"power of two" in lib.adk_last_error()
    assert vjp(T=1024) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
    assert dgrad(T=1024) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
    assert vjp(hop=0) == ADK_ERR_ARG and vjp(n=-1) == ADK_ERR_ARG and vjp(ntw=0) == ADK_ERR_ARG
    assert dgrad(nm=257) == ADK_ERR_ARG and dgrad(lb=3) == ADK_ERR_ARG
    for kw in ({"x": None}, {"g": None}, {"ws": None}, {"out": None}, {"tr": None}, {"win": None}):
        assert vjp(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"a": None}, {"b": None}, {"up": None}, {"ws": None}, {"out": None}):
        assert dgrad(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    assert vjp(out=C.c_void_p(18)) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error()
    assert vjp(g=C.c_void_p(18)) == ADK_ERR_ARG and dgrad(up=C.c_void_p(18)) == ADK_ERR_ARG
    assert dgrad(ws=C.c_void_p(18)) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error()
    assert vjp(n=0, x=None, g=None, ws=None, out=None) == 0                       # nothing to do: no launch
    assert dgrad(n=0, a=None, b=None, up=None, ws=None, out=None) == 0


def test_workspace_bytes(lib):
    """One windowed frame gradient of n_fft floats per frame and signal."""
    ws = lib.adk_mel_grad_workspace_bytes
    assert ws(0, 4800, 2048, 300) == 0
    assert ws(16, 9600, 2048, 300) == 16 * 33 * 2048 * 4
    assert ws(2, 129, 256, 32) == 2 * 5 * 256 * 4
    assert ws(256, 48000, 2048, 300) == 256 * 161 * 2048 * 4 == 337641472        # 337.6 MB
    assert ws(4096, 480000, 4096, 64) == 4096 * 7501 * 4096 * 4 > 2 ** 32         # an int64, not an int
    assert ws(1, 4800, 2048, 0) == ADK_ERR_ARG and ws(-1, 4800, 2048, 300) == ADK_ERR_ARG
    assert ws(1, 0, 2048, 300) == ADK_ERR_ARG and ws(1, 4800, 0, 300) == ADK_ERR_ARG
