"""CPU: the STFT and waveform-shape losses' backward -- host side, and what tests/golden/stft_grad.npz means.

  * the fp64 restatement (stft_grad_oracle) reproduces the reference's float32 autograd gradients stored in the fixture;
  * its sign and mask overrides work;
  * `differentiable` defaults to False everywhere and the refusal of grad inputs stays; a target may never require grad;
  * the adk_grad_stft_mag / adk_grad_stft_distance / adk_grad_shape_distance / adk_grad_stft_workspace_bytes bindings and their
    argument checks, which run on the host before any HIP call.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stft_grad_oracle as SG
import stft_oracle as SO

ADK_ERR_ARG = -1
STORED = [c for c in SG.CASES if SG.stored(c[1])]
SHAPE_ALL = SG.SHAPE_CASES + [(b, None) for b in SG.BUILT]
SHAPE_STORED = [c for c in SHAPE_ALL if c[0] in SG.BUILT or SG.stored(c[1])]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "stft_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def test_fixture_covers_every_case(fixture):
    assert len(SG.CASES) == 9 and len(STORED) == 8 and len(SHAPE_ALL) == 17 and len(SHAPE_STORED) == 12
    for pname, shape in SG.CASES:
        K, p = SG.key(pname, shape), SG.params(pname)
        n = int(np.prod(shape[:-1]))
        for r, (n_fft, hop, _) in enumerate(SO.resolutions(p)):
            # the reference's own float32 error: sc and the VJP are a few 1e-7, the log term (a sum of +-1 / x_mag) up to 3e-4
            assert 0 < float(fixture[f"{K}_relerr32_sc{r}"]) < 1e-5 and 0 < float(fixture[f"{K}_relerr32_vjp{r}"]) < 1e-5
            assert 0 < float(fixture[f"{K}_relerr32_mag{r}"]) < 1e-3
            elements = n * (1 + shape[-1] // hop) * (n_fft // 2 + 1)
            assert int(fixture[f"{K}_weak{r}"]) <= SG.WEAK_CAP * elements and int(fixture[f"{K}_fragile{r}"]) <= SG.FRAGILE_CAP
            assert int(fixture[f"{K}_signdiff{r}"]) == 0 and int(fixture[f"{K}_maskdiff{r}"]) == 0
            assert (f"{K}_vjp{r}" in fixture.files) == SG.stored(shape)
        assert (f"{K}_grad_sc" in fixture.files) == (f"{K}_grad_mag" in fixture.files) == SG.stored(shape)
    for name, shape in SHAPE_ALL:
        assert (SG.shape_key(name, shape) + "_grad" in fixture.files) == ((name, shape) in SHAPE_STORED)


@pytest.mark.parametrize("pname,shape", STORED, ids=[SG.key(*c) for c in STORED])
def test_fp64_oracle_reproduces_reference_gradients(fixture, pname, shape):
    """The stored float32 gradients against the oracle with its own signs and masks, which the fixture records to be the
    reference's on every element (signdiff = maskdiff = 0): within 4x the reference's stored float32 error, the rule the GPU test
    holds the HIP path to."""
    p, K = SG.params(pname), SG.key(pname, shape)
    y_hat, y = SG.inputs(shape)
    n, R = int(np.prod(shape[:-1])), len(p["fft_sizes"])
    wins = SG.windows_f32(p)
    for term, (us, um) in (("sc", (1.0, 0.0)), ("mag", (0.0, 1.0))):
        ref = fixture[f"{K}_grad_{term}"]
        g = SG.loss_grad64(y_hat, y, p, us, um)
        assert g.shape == ref.shape == (n, shape[-1])
        err = SG.rel_l2(ref, g)
        rel32 = max(float(fixture[f"{K}_relerr32_{term}{r}"]) for r in range(R))
        print(f"{K}: {term} gradient, reference f32 against the oracle: {err:.3g} (relerr32 {rel32:.3g})")
        assert err <= 4 * rel32 + 1e-6
    for r, (n_fft, hop, wl) in enumerate(SO.resolutions(p)):
        v = SG.mag_vjp64(y_hat, SG.upstream(pname, shape, r, p), n_fft, hop, wl, wins[r])
        err = SG.rel_l2(fixture[f"{K}_vjp{r}"], v)
        print(f"{K} r{r}: VJP, reference f32 against the oracle: {err:.3g}")
        assert err <= 4 * float(fixture[f"{K}_relerr32_vjp{r}"]) + 1e-6


@pytest.mark.parametrize("name,shape", SHAPE_STORED, ids=[SG.shape_key(*c) for c in SHAPE_STORED])
def test_shape_oracle_reproduces_reference_gradients(fixture, name, shape):
    y_hat, y, winlens = SG.shape_case(name, shape)
    ref = fixture[SG.shape_key(name, shape) + "_grad"].astype(np.float64)
    g = SG.shape_grad64(y_hat, y, winlens)
    assert np.array_equal(ref != 0, g != 0)
    # float32 autograd: a few roundings of the largest term at a sample (terms of opposite sign may meet there and cancel)
    assert (np.abs(ref - g) <= 4 * 2.0 ** -24 * SG.shape_grad64(y_hat, y, winlens, magnitude=True)).all()
    T = y.shape[-1]
    for w in winlens:                                                      # the dropped tail
        if T % w and len(winlens) == 1:
            assert not g[:, T - T % w:].any()


def test_shape_oracle_first_index_and_equal_maxima(fixture):
    y_hat, y, winlens = SG.shape_case("tie")
    assert winlens == [100, 7] and SG.shape_ties(y_hat, y, 100) == (3, 0) and SG.shape_ties(y_hat, y, 7) == (1, 0)
    g = SG.shape_grad64(y_hat, y, winlens)
    ref = fixture["shape_tie_grad"]
    for s, first, second in ((0, 310, 350), (0, 1210, 1274), (1, 700, 703)):
        assert g[s, first] != 0 and np.sign(g[s, first]) == np.sign(y_hat[s, 0, first]) == np.sign(ref[s, first])
    assert g[1, 703] == 0 == ref[1, 703]                                        # the second of a tie, in both window lengths
    # the second of a tie in its window of 100 gets nothing from it; it is alone in its window of 7 (R = 2, n = 2, 285 windows)
    assert g[0, 350] == 1.0 / (2 * 2 * 285) and g[0, 1274] == -1.0 / (2 * 2 * 285)
    assert ref[0, 350] == np.float32(g[0, 350]) and ref[0, 1274] == np.float32(g[0, 1274])
    y_hat, y, winlens = SG.shape_case("equal")
    assert SG.shape_ties(y_hat, y, 100) == (0, 2) and SG.shape_ties(y_hat, y, 7) == (0, 2)
    g = SG.shape_grad64(y_hat, y, winlens)
    assert g[0, 310] == 0 and g[1, 703] == 0 and fixture["shape_equal_grad"][0, 310] == 0
    for name, shape in SG.SHAPE_CASES:
        y_hat, y, winlens = SG.shape_case(name, shape)
        assert all(SG.shape_ties(y_hat, y, w) == (0, 0) for w in winlens)


def test_oracle_sign_and_mask_overrides_and_coverage():
    p = SG.params("gap")
    y_hat, y = SG.inputs((2, 1, 2000))
    own_s = [np.sign(d) for d in SG.dlog64(y_hat, y, p)]
    own_m = [SG.power64(y_hat, 256, 300, 256, SG.windows_f32(p)[0]) >= SG.EPS]
    g_mag, g_sc = SG.loss_grad64(y_hat, y, p, 0.0, 1.0), SG.loss_grad64(y_hat, y, p, 1.0, 0.0)
    assert np.array_equal(SG.loss_grad64(y_hat, y, p, 0.0, 1.0, signs=own_s, masks=own_m), g_mag)
    assert np.array_equal(SG.loss_grad64(y_hat, y, p, 0.0, 1.0, signs=[-s for s in own_s]), -g_mag)     # negated signs negate mag
    assert np.array_equal(SG.loss_grad64(y_hat, y, p, 1.0, 0.0, signs=[-s for s in own_s]), g_sc)       # ... and leave sc alone
    assert np.allclose(SG.loss_grad64(y_hat, y, p, 1.0, 1.0), g_sc + g_mag, rtol=1e-12, atol=0)
    none = [np.zeros_like(own_m[0])]
    assert not SG.loss_grad64(y_hat, y, p, 1.0, 1.0, masks=none).any()
    assert not own_m[0].all()                                                   # the case has a bin below eps
    cov = SG.coverage(2000, 256, 300, 256)
    assert int((cov == 0).sum()) * 2 == 684
    assert np.array_equal(g_sc == 0, np.broadcast_to(cov == 0, g_sc.shape))
    assert np.array_equal(g_mag == 0, np.broadcast_to(cov == 0, g_mag.shape))


def test_differentiable_defaults_to_false_and_refusal_stays():
    from audiodec_amd import stft_loss, waveform_loss
    assert stft_loss.STFTLoss().differentiable is False
    loss = stft_loss.MultiResolutionSTFTLoss()
    assert loss.differentiable is False and not any(f.differentiable for f in loss.stft_losses)
    cfg = {"use_stft_loss": True, "stft_loss_params": dict(SO.PARAMS["defaults"]),
           "use_shape_loss": True, "shape_loss_params": {"winlen": [300, 200]}}
    assert stft_loss.from_config(cfg).differentiable is False
    d = stft_loss.from_config(cfg, differentiable=True)
    assert d.differentiable is True and all(f.differentiable for f in d.stft_losses)
    assert stft_loss.from_config({}, differentiable=True) is None
    assert waveform_loss.WaveformShapeLoss(300).differentiable is False
    shape = waveform_loss.MultiWindowShapeLoss()
    assert shape.differentiable is False and not any(f.differentiable for f in shape.shape_losses)
    assert waveform_loss.from_config(cfg).differentiable is False
    ds = waveform_loss.from_config(cfg, differentiable=True)
    assert ds.differentiable is True and all(f.differentiable for f in ds.shape_losses) and len(ds.shape_losses) == 2
    assert waveform_loss.from_config({}, differentiable=True) is None
    x, z = torch.zeros(1, 4800, requires_grad=True), torch.zeros(1, 4800)
    for call in (lambda: loss(x, z), lambda: loss(z, x), lambda: stft_loss.STFTLoss()(x, z),
                 lambda: stft_loss.stft(x, 512, 128, 512, torch.hann_window(512)),
                 lambda: shape(x, z), lambda: shape(z, x), lambda: waveform_loss.WaveformShapeLoss(300)(x, z)):
        with pytest.raises(NotImplementedError, match="forward only"):
            call()
    # out of scope, forward only whatever is asked of the rest
    with pytest.raises(NotImplementedError, match="forward only"):
        stft_loss.SpectralConvergenceLoss()(torch.ones(1, 4, 5, requires_grad=True), torch.ones(1, 4, 5))
    with pytest.raises(NotImplementedError, match="forward only"):
        stft_loss.LogSTFTMagnitudeLoss()(torch.ones(1, 4, 5, requires_grad=True), torch.ones(1, 4, 5))


def test_target_requiring_grad_is_refused():
    from audiodec_amd import stft_loss, waveform_loss
    y, z = torch.zeros(1, 4800, requires_grad=True), torch.zeros(1, 4800)
    for loss in (stft_loss.MultiResolutionSTFTLoss(differentiable=True), stft_loss.STFTLoss(differentiable=True),
                 waveform_loss.MultiWindowShapeLoss(differentiable=True), waveform_loss.WaveformShapeLoss(100, differentiable=True)):
        with pytest.raises(NotImplementedError, match="forward only"):
            loss(z, y)
        with pytest.raises(NotImplementedError, match="forward only"):
            loss(torch.zeros(1, 4800, requires_grad=True), y)


def test_argument_errors_come_first():
    from audiodec_amd import stft_loss, waveform_loss
    short = torch.zeros(1, 500, requires_grad=True)
    with pytest.raises(ValueError, match="reflect padding"):
        stft_loss.MultiResolutionSTFTLoss(differentiable=True)(short, torch.zeros(1, 500))
    with pytest.raises(ValueError, match="reflect padding"):
        stft_loss.STFTLoss(differentiable=True)(short, torch.zeros(1, 500))
    with pytest.raises(ValueError, match="same shape"):
        stft_loss.MultiResolutionSTFTLoss(differentiable=True)(torch.zeros(1, 4800, requires_grad=True), torch.zeros(2, 4800))
    with pytest.raises(ValueError, match="reflect padding"):
        stft_loss.stft(short, 2048, 300, 2048, torch.hann_window(2048), differentiable=True)
    with pytest.raises(ValueError, match="window of win_length"):
        stft_loss.stft(torch.zeros(1, 4800, requires_grad=True), 512, 128, 512, torch.hann_window(400), differentiable=True)
    with pytest.raises(NotImplementedError, match="powers of two"):
        stft_loss.stft(torch.zeros(1, 4800, requires_grad=True), 1000, 128, 512, torch.hann_window(512), differentiable=True)
    with pytest.raises(ValueError, match="shorter than winlen"):
        waveform_loss.MultiWindowShapeLoss(differentiable=True)(torch.zeros(1, 150, requires_grad=True), torch.zeros(1, 150))
    with pytest.raises(ValueError, match="same shape"):
        waveform_loss.WaveformShapeLoss(100, differentiable=True)(torch.zeros(1, 150, requires_grad=True), torch.zeros(1, 151))


def test_grad_symbols_are_bound(lib):
    from audiodec_amd import native
    for name in ("adk_grad_stft_workspace_bytes", "adk_grad_stft_mag", "adk_grad_stft_distance", "adk_grad_shape_distance"):
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    win = np.hanning(2048).astype(np.float32)
    # host arrays stand in for device pointers: every call below must fail (or finish) before touching them
    Wn, dummy, odd = win.ctypes.data_as(C.c_void_p), C.c_void_p(16), C.c_void_p(18)

    def vjp(n=2, T=4800, n_fft=2048, hop=300, wl=2048, x=dummy, g=dummy, ws=dummy, out=dummy, win=Wn):
        return lib.adk_grad_stft_mag(x, g, n, T, n_fft, hop, win, wl, C.c_float(1e-7), ws, out, None)

    def dgrad(n=2, T=4800, n_fft=2048, hop=300, wl=2048, x=dummy, y=dummy, sums=dummy, us=dummy, um=dummy, ws=dummy, out=dummy,
              win=Wn):
        return lib.adk_grad_stft_distance(x, y, n, T, n_fft, hop, win, wl, C.c_float(1e-7), sums, 1.0, us, 1e-3, um, ws, out, None)

    def sgrad(n=2, T=4800, winlen=300, a=dummy, b=dummy, up=dummy, out=dummy):
        return lib.adk_grad_shape_distance(a, b, n, T, winlen, 1e-3, up, out, None)

    for fn in (vjp, dgrad):
        for bad in (1000, 128, 8192, 0):
            assert fn(n_fft=bad) == ADK_ERR_ARG and b"power of two" in lib.adk_last_error()
        assert fn(T=1024) == ADK_ERR_ARG and b"reflect" in lib.adk_last_error()
        assert fn(hop=0) == ADK_ERR_ARG and fn(n=-1) == ADK_ERR_ARG and fn(wl=0) == ADK_ERR_ARG and fn(wl=2049) == ADK_ERR_ARG
        assert fn(win=None) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error()
    for kw in ({"x": None}, {"g": None}, {"ws": None}, {"out": None}):
        assert vjp(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"x": None}, {"y": None}, {"sums": None}, {"us": None}, {"um": None}, {"ws": None}, {"out": None}):
        assert dgrad(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"x": odd}, {"g": odd}, {"ws": odd}, {"out": odd}):
        assert vjp(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    for kw in ({"x": odd}, {"y": odd}, {"us": odd}, {"um": odd}, {"ws": odd}, {"out": odd}, {"sums": odd},
               {"sums": C.c_void_p(20)}):                                         # sums: 8-byte
        assert dgrad(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert vjp(n=0, x=None, g=None, ws=None, out=None) == 0                       # nothing to do: no launch
    assert dgrad(n=0, x=None, y=None, sums=None, us=None, um=None, ws=None, out=None) == 0
    assert sgrad(winlen=0) == ADK_ERR_ARG and b"winlen" in lib.adk_last_error()
    assert sgrad(n=-1) == ADK_ERR_ARG and sgrad(T=299) == ADK_ERR_ARG and b"MaxPool1d" in lib.adk_last_error()
    for kw in ({"a": None}, {"b": None}, {"up": None}, {"out": None}):
        assert sgrad(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"a": odd}, {"b": odd}, {"up": odd}, {"out": odd}):
        assert sgrad(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert sgrad(n=0, a=None, b=None, up=None, out=None) == 0


def test_workspace_bytes(lib):
    """One windowed frame gradient of n_fft floats per frame and signal."""
    ws = lib.adk_grad_stft_workspace_bytes
    assert ws(0, 4800, 2048, 300) == 0
    assert ws(16, 9600, 1024, 120) == 16 * 81 * 1024 * 4
    assert ws(16, 9600, 2048, 240) == 16 * 41 * 2048 * 4
    assert ws(16, 9600, 512, 50) == 16 * 193 * 512 * 4
    assert ws(2, 257, 512, 128) == 2 * 3 * 512 * 4
    assert ws(4096, 480000, 4096, 64) == 4096 * 7501 * 4096 * 4 > 2 ** 32         # an int64, not an int
    assert ws(1, 4800, 2048, 0) == ADK_ERR_ARG and ws(-1, 4800, 2048, 300) == ADK_ERR_ARG
    assert ws(1, 0, 2048, 300) == ADK_ERR_ARG and ws(1, 4800, 0, 300) == ADK_ERR_ARG
