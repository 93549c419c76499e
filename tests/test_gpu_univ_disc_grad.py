"""GPU: the UnivNet discriminator's backward to its input (adk_conv2d_grad, adk_spectrogram_grad, the differentiable subclasses).

  A. conv op, exact: small integer-valued weights, inputs and upstream gradients make every f32 sum exact, so dx must torch.equal
     the f64 autograd of F.conv2d (+ leaky_relu(0.5)) cast to f32 -- over the shapes that can break the phase indexing;
  B. spectrogram op: against the f64 autograd of univ_disc_oracle.spectrogram64 within 4 E32 + 1e-6 max|grad64|, E32 the error of
     CPU torch float32 autograd of the same restatement; zero-magnitude bins; reproducibility into NaN-filled buffers;
  C. decisions: LeakyReLU masks and L1 signs taken from the HIP forward's feature maps differ from the fp64 ones only at elements
     whose fp64 margin is within the forward test's bound for that layer;
  D. gradient: for every case and flag set, max|hip - grad64(HIP's decisions)| <= 4 E_ref + 1e-6 max|grad64|, E_ref the
     reference's own float32 error at its own decisions (univ_disc_grad.npz);
  E. bitwise reproducibility; AdversarialEval(differentiable=True) against the forward-only call and the separate classes; graph
     construction; the all-zero resolution; flat_channel; the second backward.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import univ_disc_grad_oracle as GO
import univ_disc_oracle as UO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "univ_disc_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def forward_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "univ_disc.npz"), allow_pickle=False)


# ---- A. conv op ----
# (n_items, c_in, c_out, kernel, stride, pad or None = (k - 1) // 2, H, W, leaky, forced impl)
CONV_CASES = {
    "s12_k39_w21": (2, 4, 4, (3, 9), (1, 2), None, 5, 21, True, None),          # phases of 5 and 4 taps: K = 60 and 48
    "s12_k39_w22": (2, 4, 4, (3, 9), (1, 2), None, 5, 22, True, None),          # W + 2 pw - kw = 21: the last padded column is never read
    "s12_k39_w22_tail": (2, 4, 4, (3, 9), (1, 2), (1, 0), 5, 22, True, None),   # no padding: W - kw = 13, input column 21 is never read
    "cin32_n127": (1, 32, 6, (3, 3), (1, 1), None, 1, 127, True, None),         # one full M tile, one column short of an N tile
    "cin33_n129": (1, 33, 4, (3, 3), (1, 1), None, 3, 43, True, None),          # M tile edge, second N tile of one column
    "items_in_tile": (3, 4, 4, (3, 3), (1, 1), None, 5, 10, True, None),        # item boundaries at columns 50 and 100 of tile 0
    "plane_1x1": (1, 4, 4, (3, 9), (1, 2), None, 1, 1, True, None),
    "h1_kh3": (2, 4, 4, (3, 9), (1, 2), None, 1, 30, True, None),
    "s23_k35": (2, 4, 6, (3, 5), (2, 3), None, 7, 11, True, None),              # six phases, tails on both axes
    "s23_k35_short": (1, 4, 6, (3, 5), (2, 3), None, 1, 2, True, None),         # fewer rows and columns than phases
    "k22_s33_empty_phases": (1, 4, 6, (2, 2), (3, 3), (1, 1), 8, 10, True, None),   # kernel < stride: five phases without taps
    "cout40_k600": (1, 4, 40, (3, 9), (1, 2), None, 4, 20, True, None),         # K = 600 > 16 x 16
    "noact": (2, 8, 8, (3, 3), (1, 1), None, 6, 9, False, None),
    "first_layer_cin1": (2, 1, 32, (3, 9), (1, 1), None, 6, 40, True, None),    # direct: dx is the spectrogram's gradient
    "output_cout1": (2, 16, 1, (3, 3), (1, 1), None, 6, 20, False, None),       # direct: the output conv
    "s12_k39_w22_tail_direct": (2, 4, 4, (3, 9), (1, 2), (1, 0), 5, 22, True, "direct"),
    "s23_k35_direct": (2, 4, 6, (3, 5), (2, 3), None, 7, 11, True, "direct"),
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv2d_grad_exact(gpu, name):
    from audiodec_amd import discriminator as D
    from audiodec_amd import univnet_discriminator as U
    n, cin, cout, kernel, stride, pad, h, w, leaky, forced = CONV_CASES[name]
    pad = pad or ((kernel[0] - 1) // 2, (kernel[1] - 1) // 2)
    L = U.SpecLayer("op", cin, cout, kernel, stride, pad, True, 0.5 if leaky else None, "none")
    rng = np.random.default_rng(n + cin + cout + sum(kernel) + sum(stride) + h + w)
    wt = torch.from_numpy(rng.integers(-3, 4, size=L.weight_shape).astype(np.float32))
    b = torch.from_numpy(rng.integers(-2, 3, size=cout).astype(np.float32))
    x = torch.from_numpy(rng.integers(-4, 5, size=(n, cin, h, w)).astype(np.float32))
    ho, wo = U.conv2d_out_shape(h, w, L)
    dy = torch.from_numpy(rng.integers(-3, 4, size=(n, cout, ho, wo)).astype(np.float32))
    conv = U._Conv2d(L, wt, b, gpu)
    if forced == "direct":
        assert conv.impl == D.IMPL_GEMM
        conv.impl, conv.w = D.IMPL_DIRECT, wt.contiguous().to(gpu)
    else:
        assert conv.impl == (D.IMPL_DIRECT if cin == 1 or cout == 1 else D.IMPL_GEMM)
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(xr, wt.double(), b.double(), stride=stride, padding=pad)
    if leaky:
        yr = F.leaky_relu(yr, 0.5)
    yr.backward(dy.double())
    xg = x.to(gpu).requires_grad_(True)
    y = D._ConvFn.apply(xg, conv)
    assert y.requires_grad and torch.equal(y.detach().cpu(), yr.detach().float())
    y.backward(dy.to(gpu))
    assert xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
    assert torch.equal(xg.grad.cpu(), xr.grad.float()), f"{name}: max diff {float((xg.grad.cpu() - xr.grad.float()).abs().max())}"
    assert float(xr.grad.abs().max()) > 0
    if name.startswith("s12_k39_w22_tail"):
        assert float(xr.grad[..., -1].abs().max()) == 0 and float(xr.grad[..., -2].abs().max()) > 0


# ---- B. spectrogram op ----
def _spec_grad(x, g, window, fft, hop, win, ws=None, out=None):
    """adk_spectrogram_grad itself, into the given (or fresh) workspace and output."""
    from audiodec_amd import discriminator as D
    from audiodec_amd import native
    n, t = x.shape
    lib = native.lib()
    nbytes = int(lib.adk_spectrogram_grad_workspace_bytes(n, t, win // 2, fft, hop))
    assert nbytes == n * (1 + (t + 2 * (win // 2)) // hop) * fft * 4
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if ws is None else ws
    out = torch.empty(n, t, dtype=torch.float32, device=x.device) if out is None else out
    native.check(lib.adk_spectrogram_grad(D._ptr(x), D._ptr(g), n, t, win // 2, fft, hop, D._ptr(window), win, D._ptr(ws), D._ptr(out),
                                          native.current_stream(x.device)), "adk_spectrogram_grad")
    return out, ws


def _spec_case(fft, hop, win, t, rows):
    from audiodec_amd import synth
    x = np.stack([synth.synth_audio(UO.SEED, f"univ_disc_grad/spec/{fft}/{t}/{i}", t) for i in range(rows)]).astype(np.float32)
    frames, bins = 1 + (t + 2 * (win // 2)) // hop, fft // 2 + 1
    g = np.random.default_rng(fft + t + rows).standard_normal((rows, frames, bins)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(g), torch.hann_window(win)


# every length the reflect padding accepts: T + 2 (win // 2) > fft / 2 (univnet_discriminator.min_samples)
SPEC_CASES = [(fft, hop, win, t) for fft, hop, win in [(256, 25, 120), (512, 384, 300), (2048, 240, 1200)]
              for t in (17, 150, 301, 2310) if t + 2 * (win // 2) > fft // 2]


@pytest.mark.parametrize("fft,hop,win,t", SPEC_CASES)
def test_spectrogram_grad_against_fp64(gpu, fft, hop, win, t):
    from audiodec_amd import univnet_discriminator as U
    assert len(SPEC_CASES) == 12 and t >= U.min_samples(fft, win)
    for rows in (1, 3):
        x, g, window = _spec_case(fft, hop, win, t, rows)
        grads = {}
        for dt in (torch.float64, torch.float32):
            xr = x.clone().to(dt).requires_grad_(True)
            s = UO.spectrogram64(xr, window.to(dt), fft, hop, win)
            assert s.shape == g.shape
            s.backward(g.to(dt))
            grads[dt] = xr.grad.double()
        exact = grads[torch.float64]
        e32, gmax = float((grads[torch.float32] - exact).abs().max()), float(exact.abs().max())
        xg = x.to(gpu).requires_grad_(True)
        s = U._SpecFn.apply(xg, window.to(gpu), fft, hop, win)
        assert s.requires_grad and torch.equal(s.detach(), U.spectrogram(x.to(gpu), window.to(gpu), fft, hop, win))
        s.backward(g.to(gpu))
        assert xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
        err, bound = float((xg.grad.cpu().double() - exact).abs().max()), 4 * e32 + 1e-6 * gmax
        print(f"spec {fft}/{hop}/{win} T {t} rows {rows}: max|hip - grad64| {err:.3g}  E32 {e32:.3g}  max|grad64| {gmax:.3g}  "
              f"ratio to bound {err / bound if bound else 0.0:.3f}")
        assert err <= bound, f"max|hip - grad64| {err:.3g} > {bound:.3g}"
        # 17 samples under hop 384: the only frame is frame 0, which lies in the zero padding; the gradient is 0 and the bound is 0
        assert (gmax == 0) == ((fft, t) == (512, 17))
        direct, _ = _spec_grad(x.to(gpu), g.to(gpu), window.to(gpu), fft, hop, win)
        assert torch.equal(direct, xg.grad)


def test_spectrogram_grad_zero_magnitude(gpu):
    """|X| == 0 passes no gradient: an all-zero signal, and a signal shorter than the padding whose only frame lies in it."""
    x, g, window = _spec_case(512, 60, 300, 301, 2)
    out, _ = _spec_grad(torch.zeros_like(x).to(gpu), g.to(gpu), window.to(gpu), 512, 60, 300)
    assert torch.isfinite(out).all() and torch.equal(out, torch.zeros_like(out))
    # T = 40 < pad = 60, hop = 200: one frame, centred on position 0 of the padded signal; its window covers [-60, 60), all zeros
    x, g, window = _spec_case(256, 200, 120, 40, 3)
    assert g.shape[1] == 1
    xr = x.double().requires_grad_(True)
    s = UO.spectrogram64(xr, window.double(), 256, 200, 120)
    assert float(s.detach().abs().max()) == 0
    s.backward(g.double())
    assert torch.equal(xr.grad, torch.zeros_like(xr.grad))
    out, _ = _spec_grad(x.to(gpu), g.to(gpu), window.to(gpu), 256, 200, 120)
    assert torch.isfinite(out).all() and torch.equal(out, torch.zeros_like(out))


def test_spectrogram_grad_reproducible_into_nan_buffers(gpu):
    x, g, window = _spec_case(256, 25, 120, 301, 3)
    x, g, window = x.to(gpu), g.to(gpu), window.to(gpu)
    first, ws = _spec_grad(x, g, window, 256, 25, 120)
    again, _ = _spec_grad(x, g, window, 256, 25, 120, ws=torch.full_like(ws, float("nan")), out=torch.full_like(first, float("nan")))
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))


# ---- C, D: the whole network ----
_DISCS, _STATE = {}, {}


def _disc(pname, gpu, differentiable=True):
    from audiodec_amd import univnet_discriminator as U
    key = (pname, differentiable)
    if key not in _DISCS:
        cls = U.DifferentiableDiscriminator if differentiable else U.Discriminator
        _DISCS[key] = cls(**UO.PARAMS[pname], device=gpu).load_state_dict(UO.state_dict(pname))
    return _DISCS[key]


def _eval(pname, flags, gpu, differentiable=True):
    from audiodec_amd import univnet_discriminator as U
    return U.from_config(GO.eval_config(flags), _disc(pname, gpu, differentiable), differentiable=differentiable)


def _state(case, gpu):
    """Per case, once: the inputs, the HIP forward's feature maps' decisions, and the fp64 feature maps' decisions and margins."""
    if case not in _STATE:
        pname = GO.CASES[case][0]
        y_hat, y = GO.inputs(case)
        sd = UO.state_dict(pname)
        with torch.no_grad():
            d = _disc(pname, gpu)
            hip_hat = [[t.cpu().numpy() for t in o] for o in d(torch.from_numpy(y_hat).to(gpu))]
            hip = [[t.cpu().numpy() for t in o] for o in d(torch.from_numpy(y).to(gpu))]
            f64_hat = [[GO._np(t) for t in o] for o in GO.features64(pname, sd, torch.from_numpy(y_hat).double())]
            f64 = [[GO._np(t) for t in o] for o in GO.features64(pname, sd, torch.from_numpy(y).double())]
        _STATE[case] = dict(pname=pname, sd=sd, y_hat=y_hat, y=y, hip=GO.decisions(hip_hat, hip), f64=GO.decisions(f64_hat, f64),
                            margins=GO.margins64(f64_hat, f64), f64_cat=[[np.concatenate([a, b], 0) for a, b in zip(oh, o)]
                                                                         for oh, o in zip(f64_hat, f64)])
    return _STATE[case]


def _hip_grad(case, flags, gpu):
    st = _state(case, gpu)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    v = _eval(st["pname"], flags, gpu)(a, torch.from_numpy(st["y"]).to(gpu))
    (GO.UPSTREAM * v["adversarial_loss"]).backward()
    return v, a.grad


@pytest.mark.parametrize("case", list(GO.CASES))
def test_decisions_differ_from_fp64_only_within_the_forward_bound(gpu, fixture, forward_fixture, case):
    st = _state(case, gpu)
    if case in GO.FULL_CASES:
        bounds = fixture[f"{case}_bounds"]
    else:                                            # from the stored samples, as the forward test does
        bounds = []
        for d, o in enumerate(st["f64_cat"]):
            for l, t in enumerate(o):
                ex = t.reshape(-1)[UO.sample_index(t.size)]
                ref = forward_fixture[f"{case}_d{d}_l{l}_sample"]
                bounds.append(4 * np.max(np.abs(ref - ex)) + 1e-6 * max(1.0, float(np.max(np.abs(ex)))))
    found, ok = GO.disagreements(*st["hip"], *st["f64"], st["margins"], bounds)
    for d, l, what, n, worst, bound in found:
        print(f"{case} d{d} l{l}: {n} {what} decisions differ from fp64, worst fp64 margin {worst:.3g}, bound {bound:.3g}")
    print(f"{case}: {sum(f[3] for f in found)} decisions differ from fp64")
    assert ok, f"{case}: a HIP decision differs from fp64 at an element outside the forward bound: {found}"


@pytest.mark.parametrize("flags", list(GO.FLAGS))
@pytest.mark.parametrize("case", list(GO.CASES))
def test_gradient_against_fp64_at_hip_decisions(gpu, fixture, case, flags):
    st = _state(case, gpu)
    v, grad = _hip_grad(case, flags, gpu)
    assert grad.shape == st["y_hat"].shape and grad.dtype == torch.float32 and v["adversarial_loss"].requires_grad
    assert torch.isfinite(grad).all()
    exact = GO.grad64(st["pname"], st["sd"], st["y_hat"], st["y"], flags, *st["hip"])
    eref, gmax = float(fixture[f"{case}_{flags}_eref"]), float(fixture[f"{case}_{flags}_gmax"])
    err, bound = float(np.max(np.abs(grad.cpu().numpy().astype(np.float64) - exact))), 4 * eref + 1e-6 * gmax
    print(f"{case} {flags}: max|hip - grad64| {err:.3g}  E_ref {eref:.3g}  max|grad64| {gmax:.3g}  ratio to bound {err / bound:.3f}")
    assert err <= bound, f"{case} {flags}: max|hip - grad64| {err:.3g} > {bound:.3g}"


# ---- E ----
def test_bitwise_reproducible(gpu):
    for flags in ("shipped", "hinge_avg"):
        (v1, g1), (v2, g2) = _hip_grad("t2310", flags, gpu), _hip_grad("t2310", flags, gpu)
        assert torch.equal(g1, g2) and all(torch.equal(v1[k], v2[k]) for k in v1) and len(v1) == 4
        assert float(g1.abs().max()) > 0 and torch.isfinite(g1).all()


@pytest.mark.parametrize("case", ["t301", "stereo", "b2"])
def test_adversarial_eval_values_are_the_forward_only_ones(gpu, case):
    st = _state(case, gpu)
    a, b = torch.from_numpy(st["y_hat"]).to(gpu), torch.from_numpy(st["y"]).to(gpu)
    for flags in GO.FLAGS:
        with torch.no_grad():
            plain = _eval(st["pname"], flags, gpu, differentiable=False)(a, b)
            quiet = _eval(st["pname"], flags, gpu)(a.clone().requires_grad_(True), b)      # no_grad: the forward-only pass
        v = _eval(st["pname"], flags, gpu)(a.clone().requires_grad_(True), b)
        assert list(v) == list(plain) and set(v) == set(quiet)
        for k in v:
            assert v[k].dim() == 0 and v[k].dtype == torch.float32
            assert float(v[k].detach()) == pytest.approx(float(plain[k]), rel=1e-6), f"{flags} {k}"
            assert torch.equal(quiet[k], plain[k]) and not quiet[k].requires_grad
            assert v[k].requires_grad == (k in ("adversarial_loss", "feature_matching_loss")), k
        # an input that does not require grad: the plain forward
        w = _eval(st["pname"], flags, gpu)(a, b)
        assert all(torch.equal(w[k], plain[k]) and not w[k].requires_grad for k in w)


@pytest.mark.parametrize("flags", list(GO.FLAGS))
def test_adversarial_eval_gradient_is_the_separate_classes(gpu, fixture, flags):
    from audiodec_amd import univnet_discriminator as U
    st = _state("b2", gpu)
    _, g_eval = _hip_grad("b2", flags, gpu)
    f = GO.FLAGS[flags]
    d = _disc("reduced", gpu)
    a, b = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True), torch.from_numpy(st["y"]).to(gpu)
    with torch.no_grad():
        p = d(b)
    p_ = d(a)
    assert all(t.grad_fn is not None for o in p_ for t in o) and all(not t.requires_grad for o in p for t in o)
    loss = U.GeneratorAdversarialLoss(*f["gen"], differentiable=True)(p_)
    if f["fm"] is not None:
        loss = loss + f["lambda_feat_match"] * U.FeatureMatchLoss(*f["fm"], differentiable=True)(p_, p)
    assert loss.requires_grad and loss.dtype == torch.float32
    (GO.UPSTREAM * f["lambda_adv"] * loss).backward()
    gmax = float(fixture[f"b2_{flags}_gmax"])
    # the same kernels on the same decisions; the scalar factors are rounded in a different order (a few f32 roundings per term)
    assert float((a.grad - g_eval).abs().max()) <= 1e-6 * gmax
    with pytest.raises(NotImplementedError, match="forward only"):
        U.GeneratorAdversarialLoss(*f["gen"])(d(a))


def test_graph_only_when_asked(gpu):
    st = _state("t301", gpu)
    d, plain = _disc("reduced", gpu), _disc("reduced", gpu, differentiable=False)
    a = torch.from_numpy(st["y_hat"]).to(gpu)
    outs = d(a)                                                                    # does not require grad: no graph
    assert all(t.grad_fn is None and not t.requires_grad for o in outs for t in o)
    with torch.no_grad():
        quiet = d(a.clone().requires_grad_(True))
        ref = plain(a)
    graph = d(a.clone().requires_grad_(True))
    assert len(outs) == len(ref) == 8
    for o, q, r, gph in zip(outs, quiet, ref, graph):
        for t, u, v, w in zip(o, q, r, gph):
            assert torch.equal(t, v) and torch.equal(u, v) and torch.equal(w.detach(), v)
            assert not u.requires_grad and w.grad_fn is not None
    for call in (plain, plain.mrsd, plain.mrsd.discriminators[0]):
        with pytest.raises(NotImplementedError, match="forward only"):
            call(a.clone().requires_grad_(True))
    # a spectral child by itself, and a feature map's own gradient added to the gradient of what follows it
    x = a.clone().requires_grad_(True)
    o = d.mrsd.discriminators[0](x)[0]
    (o[2].sum() + o[-1].sum()).backward()
    g_both = x.grad.clone()
    x.grad = None
    d.mrsd.discriminators[0](x)[0][2].sum().backward()
    g_mid = x.grad.clone()
    x.grad = None
    d.mrsd.discriminators[0](x)[0][-1].sum().backward()
    assert float(g_both.abs().max()) > 0
    assert float((g_both - (g_mid + x.grad)).abs().max()) <= 1e-5 * float(g_both.abs().max())


def test_all_zero_resolution_gives_a_finite_gradient(gpu):
    """t128: every frame of the 1024-point resolution lies in the zero padding; its spectrogram is 0 and passes no gradient."""
    st = _state("t128", gpu)
    d = _disc("reduced", gpu)
    sub = d.mrsd.discriminators[1]
    assert sub.fft_size == 1024
    x = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    from audiodec_amd import univnet_discriminator as U
    with torch.no_grad():
        spec = U.spectrogram(x.detach()[:, 0], d._windows[sub.window_key], sub.fft_size, sub.hop_size, sub.win_length)
    assert float(spec.abs().max()) == 0
    outs = sub(x)[0]
    sum((t * t).sum() for t in outs).backward()
    assert torch.equal(x.grad, torch.zeros_like(x.grad))
    for flags in GO.FLAGS:
        _, g = _hip_grad("t128", flags, gpu)
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_stereo_with_flat_channel(gpu):
    st = _state("stereo", gpu)
    assert st["y_hat"].shape == (1, 2, 101) and _disc("flat", gpu).flat_channel
    _, g = _hip_grad("stereo", "shipped", gpu)
    assert g.shape == (1, 2, 101) and float(g[:, 0].abs().max()) > 0 and float(g[:, 1].abs().max()) > 0
    # each channel is an item of its own: the gradient of channel 0 does not depend on channel 1's values
    d = _disc("flat", gpu)
    a = torch.from_numpy(st["y_hat"]).to(gpu)
    x = a.clone().requires_grad_(True)
    sum(o[-1].sum() for o in d(x)).backward()
    b = a.clone()
    b[:, 1] = a[:, 1].flip(-1)
    z = b.requires_grad_(True)
    sum(o[-1].sum() for o in d(z)).backward()
    assert torch.equal(x.grad[:, 0], z.grad[:, 0]) and not torch.equal(x.grad[:, 1], z.grad[:, 1])


def test_double_backward(gpu):
    st = _state("t301", gpu)
    b = torch.from_numpy(st["y"]).to(gpu)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    v = _eval("reduced", "shipped", gpu)(a, b)["adversarial_loss"]
    (g,) = torch.autograd.grad(v, a, create_graph=True)
    assert not g.requires_grad                                   # the gradient is a constant to autograd
    with pytest.raises(RuntimeError, match="does not require grad"):
        g.sum().backward()
    # an upstream gradient that itself requires grad asks for the second derivative: once_differentiable's error
    w = torch.ones((), device=gpu, requires_grad=True)
    a = torch.from_numpy(st["y_hat"]).to(gpu).requires_grad_(True)
    (g,) = torch.autograd.grad(_eval("reduced", "shipped", gpu)(a, b)["adversarial_loss"] * w, a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
