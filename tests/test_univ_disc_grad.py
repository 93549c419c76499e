"""CPU: the UnivNet discriminator's backward to its input -- host side, and what tests/golden/univ_disc_grad.npz means.

  * adk_conv2d_grad / adk_spectrogram_grad_workspace_bytes / adk_spectrogram_grad are in the header and bound, the ABI is still 14,
    and their argument checks run on the host before any HIP call;
  * the backward GEMM's 2-D phase weight packing against fp64 F.conv2d autograd, walked in NumPy the way the kernel walks it;
  * the differentiable subclasses exist with their bases' arguments and state-dict keys, the bases still lack the flag, the
    factories default to today's types, and the refusals stay;
  * the fixture's reference gradients lie within their stored E_ref of the fp64 oracle at the reference's decisions, and the oracle
    with fp64 decisions is plain fp64 autograd of univ_disc_oracle's formulas.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import univ_disc_grad_oracle as GO
import univ_disc_oracle as UO
from audiodec_amd import discriminator as D
from audiodec_amd import univnet_discriminator as U

ADK_ERR_ARG, ADK_ERR_SHAPE = -1, -2
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "univ_disc_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def test_symbols_in_header_and_bound(lib):
    from audiodec_amd import native
    header = open(os.path.join(ROOT, "include", "audiodec_hip.h")).read()
    for name, ret in (("adk_conv2d_grad", "int"), ("adk_spectrogram_grad_workspace_bytes", "int64_t"), ("adk_spectrogram_grad", "int")):
        assert f"{ret} {name}(" in header
        assert name in native.SYMBOLS and getattr(lib, name) is not None
    assert "#define ADK_ABI_VERSION 14" in header and lib.adk_abi_version() == 14 and native.ABI_VERSION == 14


def test_argument_validation_without_device(lib):
    dummy, odd = C.c_void_p(16), C.c_void_p(18)      # never dereferenced: every call below fails (or finishes) before a launch

    def conv(dy=dummy, y=dummy, w=dummy, dx=dummy, n=2, cin=8, h=20, wi=30, cout=16, kh=3, kw=9, sh=1, sw=2, ph=1, pw=4, act=2,
             slope=0.2, impl=2):
        return lib.adk_conv2d_grad(dy, y, w, dx, n, cin, h, wi, cout, kh, kw, sh, sw, ph, pw, act, C.c_float(slope), impl, None)

    def spec(x=dummy, g=dummy, n=2, t=300, pad=60, n_fft=256, hop=25, window=dummy, win=120, ws=dummy, grad=dummy):
        return lib.adk_spectrogram_grad(x, g, n, t, pad, n_fft, hop, window, win, ws, grad, None)

    assert conv(n=0, dy=None, y=None, w=None, dx=None) == 0                      # nothing to do: no launch
    for kw in ({"n": -1}, {"cin": 0}, {"h": 0}, {"wi": 0}, {"cout": 0}, {"kh": 0}, {"kw": 0}, {"sh": 0}, {"sw": 0}, {"ph": -1},
               {"pw": -1}, {"kh": 40000}):
        assert conv(**kw) == ADK_ERR_ARG, kw
    assert conv(act=1) == ADK_ERR_ARG and conv(impl=3) == ADK_ERR_ARG and conv(impl=0) == ADK_ERR_ARG
    assert conv(slope=-0.1) == ADK_ERR_ARG and b"slope >= 0" in lib.adk_last_error()
    assert conv(slope=-0.1, act=0, n=0) == 0                                      # no activation: the slope is not read
    assert conv(h=1, kh=5, ph=1) == ADK_ERR_SHAPE and b"larger than the padded input" in lib.adk_last_error()
    assert conv(wi=2, kw=9, pw=3) == ADK_ERR_SHAPE
    for kw in ({"dy": None}, {"y": None}, {"w": None}, {"dx": None}):
        assert conv(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"dy": odd}, {"y": odd}, {"w": odd}, {"dx": odd}):
        assert conv(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    assert conv(cout=152, kh=3, kw=9) == ADK_ERR_ARG and b"4096" in lib.adk_last_error()      # 4104 rows
    assert conv(cout=152, kh=3, kw=9, n=0, impl=1) == 0                             # the direct kernel has no table
    assert conv(sh=300, sw=300) == ADK_ERR_ARG and b"too large" in lib.adk_last_error()
    assert conv(n=0, cout=151, kh=3, kw=9) == 0                                     # 4077 rows fit

    assert spec(n=0, x=None, g=None, ws=None, grad=None) == 0
    for kw in ({"n": -1}, {"t": 0}, {"pad": -1}, {"n_fft": 128}, {"n_fft": 8192}, {"n_fft": 300}, {"hop": 0}, {"win": 0}, {"win": 257}):
        assert spec(**kw) == ADK_ERR_ARG, kw
    assert spec(t=8, pad=60) == ADK_ERR_ARG and b"reflect padding" in lib.adk_last_error()   # 8 + 120 <= 128
    assert spec(t=2 ** 31 - 100, pad=60) == ADK_ERR_ARG and b"too long" in lib.adk_last_error()
    assert spec(window=None) == ADK_ERR_ARG and b"null window" in lib.adk_last_error()
    for kw in ({"x": None}, {"g": None}, {"ws": None}, {"grad": None}):
        assert spec(**kw) == ADK_ERR_ARG and b"null pointer" in lib.adk_last_error(), kw
    for kw in ({"x": odd}, {"g": odd}, {"window": odd}, {"ws": odd}, {"grad": odd}):
        assert spec(**kw) == ADK_ERR_ARG and b"aligned" in lib.adk_last_error(), kw
    wsb = lib.adk_spectrogram_grad_workspace_bytes
    assert wsb(3, 300, 60, 256, 25) == 3 * (1 + 420 // 25) * 256 * 4 and wsb(0, 300, 60, 256, 25) == 0
    assert wsb(2, 2 ** 31 - 1, 600, 4096, 1) == 2 * (2 ** 31 + 1200) * 4096 * 4                 # 64-bit
    for args in ((-1, 300, 60, 256, 25), (1, 0, 60, 256, 25), (1, 300, -1, 256, 25), (1, 300, 60, 0, 25), (1, 300, 60, 256, 0)):
        assert wsb(*args) == ADK_ERR_ARG, args


def _conv2d_grad_by_packing(packed, dy, L, h_in, w_in):
    """dx (C_in, H, W) of one item from the PACKED weights alone, the way the kernel walks them (numpy, float64)."""
    (kh, kw), (sh, sw), (ph, pw) = L.kernel, L.stride, L.pad
    h_out, w_out = dy.shape[1:]
    dx = np.zeros((L.cin, h_in, w_in))
    off = 0
    for rh in range(sh):
        for rw in range(sw):
            nth, ntw = len(range(rh, kh, sh)), len(range(rw, kw, sw))
            block = packed[off:off + L.cout * nth * ntw]                            # [kk = (co * nth + tth) * ntw + ttw][m]
            off += L.cout * nth * ntw
            for h in range(h_in):
                for w in range(w_in):
                    if (h + ph) % sh != rh or (w + pw) % sw != rw:
                        continue
                    uh, uw = (h + ph) // sh, (w + pw) // sw
                    for co in range(L.cout):
                        for tth in range(nth):
                            for ttw in range(ntw):
                                ho, wo = uh - tth, uw - ttw
                                if 0 <= ho < h_out and 0 <= wo < w_out:
                                    dx[:, h, w] += block[(co * nth + tth) * ntw + ttw] * dy[co, ho, wo]
    assert off == L.cout * kh * kw == packed.shape[0]
    return dx


@pytest.mark.parametrize("cin,cout,kernel,stride,h,w", [(3, 4, (3, 9), (1, 2), 5, 12), (3, 4, (3, 9), (1, 2), 4, 13),
                                                        (2, 3, (3, 5), (2, 3), 6, 10), (2, 3, (2, 2), (3, 3), 8, 7),
                                                        (3, 2, (3, 3), (3, 3), 7, 9), (4, 2, (3, 3), (1, 1), 4, 5)])
def test_phase_weight_packing(cin, cout, kernel, stride, h, w):
    pad = ((kernel[0] - 1) // 2, (kernel[1] - 1) // 2)
    L = U.SpecLayer("x", cin, cout, kernel, stride, pad, True, None, "none")
    rng = np.random.default_rng(kernel[1] * 100 + stride[1] * 10 + w)
    wt = torch.from_numpy(rng.integers(-4, 5, size=L.weight_shape).astype(np.float32))
    packed = U.pack_grad_weights2d(wt, L)
    assert tuple(packed.shape) == (cout * kernel[0] * kernel[1], cin) and packed.is_contiguous()
    ho, wo = U.conv2d_out_shape(h, w, L)
    dy = rng.integers(-3, 4, size=(cout, ho, wo)).astype(np.float64)
    x = torch.zeros(1, cin, h, w, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, wt.double(), None, stride=stride, padding=pad).backward(torch.from_numpy(dy)[None])
    assert float(x.grad.abs().max()) > 0
    assert np.array_equal(_conv2d_grad_by_packing(packed.numpy().astype(np.float64), dy, L, h, w), x.grad[0].numpy())


def test_subclasses_factories_and_refusals():
    pairs = ((U.DifferentiableSpectralDiscriminator, U.UnivNetSpectralDiscriminator),
             (U.DifferentiableMultiResolutionSpectralDiscriminator, U.UnivNetMultiResolutionSpectralDiscriminator),
             (U.DifferentiableDiscriminator, U.Discriminator))
    for sub, base in pairs:
        assert issubclass(sub, base) and sub is not base
        assert "differentiable" not in inspect.signature(base.__init__).parameters
    p = UO.PARAMS["reduced"]
    u, ud = U.Discriminator(**p), U.DifferentiableDiscriminator(**p)
    assert not hasattr(u, "differentiable") and not hasattr(u.mrsd, "differentiable") and u.mpd.differentiable is False
    assert all(not hasattr(d, "differentiable") and type(d) is U.UnivNetSpectralDiscriminator for d in u.mrsd.discriminators)
    assert ud.differentiable is True and ud.mrsd.differentiable is True and ud.mpd.differentiable is True
    assert type(ud.mrsd) is U.DifferentiableMultiResolutionSpectralDiscriminator
    assert all(type(d) is U.DifferentiableSpectralDiscriminator and d.differentiable is True for d in ud.mrsd.discriminators)
    assert ud.state_dict_keys() == u.state_dict_keys() and ud.discriminator_layers == u.discriminator_layers
    ud.load_state_dict(UO.state_dict("reduced"))                                   # strict, the window buffers included
    s, sdiff = U.UnivNetSpectralDiscriminator(512, 384, 300, channels=2), U.DifferentiableSpectralDiscriminator(512, 384, 300, channels=2)
    assert sdiff.state_dict_keys() == s.state_dict_keys() and sdiff.differentiable is True
    m = U.DifferentiableMultiResolutionSpectralDiscriminator(fft_sizes=[512, 256], hop_sizes=[60, 25], win_lengths=[300, 120])
    assert m.state_dict_keys() == U.UnivNetMultiResolutionSpectralDiscriminator(fft_sizes=[512, 256], hop_sizes=[60, 25],
                                                                               win_lengths=[300, 120]).state_dict_keys()
    # the factories
    for f in (U.discriminator_for, U.load_discriminator):
        assert inspect.signature(f).parameters["differentiable"].default is False
    for mt in ("symAudioDecUniv", "UnivNet"):
        assert type(U.discriminator_for(mt, p)) is U.Discriminator
        assert type(U.discriminator_for(mt, p, differentiable=True)) is U.DifferentiableDiscriminator
    import disc_oracle as DO
    for mt in ("symAudioDec", "HiFiGAN"):
        d0, d1 = U.discriminator_for(mt, DO.PARAMS["reduced"]), U.discriminator_for(mt, DO.PARAMS["reduced"], differentiable=True)
        assert type(d0) is D.Discriminator and d0.differentiable is False and type(d1) is D.Discriminator and d1.differentiable is True
    with pytest.raises(NotImplementedError):
        U.discriminator_for("other", {}, differentiable=True)
    cfg = GO.eval_config("shipped")
    assert U.from_config(cfg, ud, differentiable=True).differentiable is True and U.from_config(cfg, u).differentiable is False
    # the refusals stay
    x = torch.zeros(1, 1, 2310, requires_grad=True)
    for call in (lambda: u(x), lambda: u.mrsd(x), lambda: u.mrsd.discriminators[0](x), lambda: u.mpd(x)):
        with pytest.raises(NotImplementedError, match="forward only"):
            call()
    # a negative slope has no output-side mask; a layer beyond the backward's tap table
    spec_params = p["spectral_discriminator_params"]
    bad = dict(p, spectral_discriminator_params=dict(spec_params, nonlinear_activation_params={"negative_slope": -0.1}))
    U.Discriminator(**bad)
    with pytest.raises(ValueError, match="negative_slope >= 0"):
        U.DifferentiableDiscriminator(**bad)
    wide = dict(p, spectral_discriminator_params=dict(p["spectral_discriminator_params"], channels=152))     # 152 * 27 = 4104
    with pytest.raises(NotImplementedError, match="4096"):
        U.DifferentiableDiscriminator(**wide)
    U.DifferentiableDiscriminator(**dict(p, spectral_discriminator_params=dict(p["spectral_discriminator_params"], channels=151)))


def test_fixture_contents(fixture):
    assert list(GO.CASES) == ["t2310", "t301", "t128", "overlap", "stereo", "tmin", "b2", "v3"]
    assert list(GO.FLAGS) == ["shipped", "hinge_avg", "mse_nofm"]
    for case, (pname, shape) in GO.CASES.items():
        for flags in GO.FLAGS:
            ref = fixture[f"{case}_{flags}_grad"]
            assert ref.shape == tuple(shape) and ref.dtype == np.float32 and np.isfinite(ref).all()
            eref, gmax = float(fixture[f"{case}_{flags}_eref"]), float(fixture[f"{case}_{flags}_gmax"])
            assert 0 < eref <= 1e-5 * gmax, f"{case} {flags}: E_ref {eref:.3g} against max|grad64| {gmax:.3g}"
        assert (f"{case}_bounds" in fixture.files) == (f"{case}_flips" in fixture.files) == (case in GO.FULL_CASES)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "univ_disc_grad.npz")) < 1 << 20


def _reference_decisions(fixture, fwd, case):
    """The reference's float32 decisions, rebuilt from its feature maps in the forward fixture (None: that fixture has no such
    case, and the gradient fixture must record that the reference decided as fp64 does)."""
    pname = GO.CASES[case][0]
    if case not in UO.CASES:
        assert int(fixture[f"{case}_flips"]) == 0
        return None, None
    y_hat, _ = GO.inputs(case)
    n = y_hat.shape[0] * (y_hat.shape[1] if UO.PARAMS[pname].get("flat_channel", False) else 1)
    n_l = [len(ls) for ls in U.Discriminator(**UO.PARAMS[pname]).discriminator_layers]
    ref = [[fwd[f"{case}_d{d}_l{l}"] for l in range(k)] for d, k in enumerate(n_l)]
    return GO.decisions([[t[:n] for t in o] for o in ref], [[t[n:] for t in o] for o in ref])


@pytest.mark.parametrize("case", ["t301", "t128", "stereo", "tmin", "b2"])
def test_reference_gradient_within_eref_of_oracle(fixture, golden_dir, case):
    """Self-consistency: the stored float32 gradient lies within the stored E_ref of grad64 at the reference's decisions."""
    fwd = np.load(os.path.join(golden_dir, "univ_disc.npz"), allow_pickle=False)
    pname = GO.CASES[case][0]
    sd = UO.state_dict(pname)
    y_hat, y = GO.inputs(case)
    masks, signs = _reference_decisions(fixture, fwd, case)
    for flags in GO.FLAGS:
        g = GO.grad64(pname, sd, y_hat, y, flags, masks, signs)
        ref_g = fixture[f"{case}_{flags}_grad"].astype(np.float64)
        err, eref = float(np.max(np.abs(ref_g - g))), float(fixture[f"{case}_{flags}_eref"])
        print(f"{case} {flags}: max|ref - grad64| {err:.3g}  stored E_ref {eref:.3g}")
        assert g.shape == ref_g.shape and np.isfinite(g).all()
        assert err <= eref * (1 + 1e-9) + 1e-18
        assert float(np.max(np.abs(g))) == pytest.approx(float(fixture[f"{case}_{flags}_gmax"]), rel=1e-12)


@pytest.mark.parametrize("case", ["t301", "stereo"])
def test_bounds_are_the_forward_tests(fixture, golden_dir, case):
    fwd = np.load(os.path.join(golden_dir, "univ_disc.npz"), allow_pickle=False)
    pname = GO.CASES[case][0]
    y_hat, y = GO.inputs(case)
    exact = UO.forward64(pname, UO.state_dict(pname), np.concatenate([y_hat, y], 0))
    ref = [[fwd[f"{case}_d{d}_l{l}"] for l in range(len(o))] for d, o in enumerate(exact)]
    assert np.allclose(fixture[f"{case}_bounds"], GO.layer_bounds(ref, exact), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", ["t128", "stereo"])
def test_oracle_with_fp64_decisions_is_plain_autograd(case):
    pname = GO.CASES[case][0]
    sd = UO.state_dict(pname)
    y_hat, y = GO.inputs(case)
    for flags in GO.FLAGS:
        a, b = GO.grad64(pname, sd, y_hat, y, flags), GO.plain_grad64(pname, sd, y_hat, y, flags)
        assert a.shape == y_hat.shape and np.isfinite(b).all() and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


def test_zero_magnitude_bins_pass_no_gradient():
    """The rule the HIP spectrogram backward restates: an all-zero frame (frame 0 of every signal, the whole 1024-point spectrogram
    of t128) has magnitude exactly 0 and torch's abs backward gives it gradient 0, not NaN."""
    y_hat, _ = GO.inputs("t128")
    x = torch.from_numpy(y_hat[:, 0]).double().requires_grad_(True)
    win = torch.hann_window(600, dtype=torch.float64)
    s = UO.spectrogram64(x, win, 1024, 768, 600)
    assert float(s.detach().abs().max()) == 0.0
    s.sum().backward()
    assert torch.equal(x.grad, torch.zeros_like(x.grad))
    x.grad = None
    s = UO.spectrogram64(x, torch.hann_window(300, dtype=torch.float64), 512, 384, 300)
    assert float(s.detach()[:, 0].abs().max()) == 0.0 and float(s.detach().abs().max()) > 0
    s.sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
