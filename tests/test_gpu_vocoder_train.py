"""GPU: the trainable vocoder (adk_voc_*; audiodec_amd/vocoder_train.py).

  A. op level, exact: small integer x, w, dy and a power-of-two slope make every f32 sum exact, so all seven calls must torch.equal
     the f64 torch restatement cast to f32 -- grouped and one-group stride-1 convs, transposed convs, the direct kernel, a split
     weight gradient, n_items == 0 -- over the shapes at which a group or tile boundary can go wrong, with and without bias,
     res / dres and db, on outputs and a workspace full of NaN;
  B. group isolation: NaN in group 1's input (or dy) leaves groups 0 and 2 of y, dx and dw finite and bitwise what they were;
  C. equivalence: with one group and act 0 or 1 each new call is bitwise its existing counterpart;
  D. real values and real slopes (0.1, 0.01), negative side included, against f64, bound 4 E + 1e-6 max, E the error of torch's own
     f32 CPU run of the same op computed here;
  E. whole vocoder: every case of vocoder_train_*.npz within 4 E_ref + 1e-6 max of the f64 reference: y, dc and every parameter's
     sampled gradient, weight_g and weight_v included; the no_grad output against the inference path;
  F. reproducibility, accumulation, the stage-2 step, launch counts, the second backward.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_oracle as DO
import make_decoder_train_golden as MTG
import make_forward_golden as MFG
import make_vocoder_train_golden as MVG
from audiodec_amd import synth

pytestmark = pytest.mark.gpu
WAVE_TOL = 1e-4
NONE, ELU, LEAKY = 0, 1, 2
DIRECT, GEMM = 1, 2


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def _real(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _nan(gpu, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _act(x, act, alpha):
    return F.leaky_relu(x, alpha) if act == LEAKY else F.elu(x, alpha) if act == ELU else x


# ---- the layers restated in torch ops (any dtype), and their gradients by autograd ----
def _conv_ref(x, w, b, res, k, d, G, act, alpha):
    """CausalConv1d.forward (layers/conv_layer.py:146-149) on a(x), plus the skip."""
    y = F.conv1d(F.pad(_act(x, act, alpha), ((k - 1) * d, 0)), w, b, dilation=d, groups=G)
    return y if res is None else y + res


def _convtr_ref(x, w, b, s, act, alpha):
    """CausalConvTranspose1d.forward (layers/conv_layer.py:189-192) on a(x) for kernel 2s."""
    return F.conv_transpose1d(F.pad(_act(x, act, alpha), (1, 0), mode="replicate"), w, b, stride=s)[:, :, s:-s]


def _ref_all(fwd, x, w, b, dy, dres, dt):
    """(y, dx [+ dres], dw, db) of fwd(x, w, b) in dtype dt on the CPU."""
    xr, wr = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
    br = b.to(dt).requires_grad_(True) if b is not None else None
    y = fwd(xr, wr, br)
    y.backward(dy.to(dt))
    dx = xr.grad if dres is None else xr.grad + dres.to(dt)
    db = br.grad if b is not None else dy.to(dt).sum((0, 2))
    return y.detach(), dx, wr.grad, db


# ---- the native calls, on outputs and a workspace full of NaN ----
def _lib():
    from audiodec_amd import native
    return native.lib(), native


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _conv_calls(gpu, x, w, b, res, dy, dres, k, d, G, act, alpha, impl=GEMM, want_db=True, voc=True):
    """adk_voc_conv, adk_voc_conv_grad, adk_voc_conv_wgrad (or, voc=False, the existing adk_dec_conv, adk_dec_conv_grad,
    adk_conv_wgrad) -> (y, dx, dw, db)."""
    from audiodec_amd import vocoder_train as VT
    from audiodec_amd import encoder_grad as EG
    lib, native = _lib()
    n, cin, t = x.shape
    cout = w.shape[0]
    xg, wg_, bg, rg, dyg, drg = (a.to(gpu).contiguous() if a is not None else None for a in (x, w, b, res, dy, dres))
    wf = wg_.clone() if impl == DIRECT else VT.pack_conv(wg_, G)
    wb = VT.pack_conv_grad(wg_, G)
    y, dx, dw = _nan(gpu, n, cout, t), _nan(gpu, n, cin, t), _nan(gpu, *w.shape)
    db = _nan(gpu, cout) if want_db else None
    st, fa = native.current_stream(gpu), C.c_float(alpha)
    xa = xg if act != NONE else None
    if voc:
        nb, _ = VT.conv_wgrad_plan(n, cin, t, cout, k, d, G)
        ws = _nan(gpu, max(1, nb // 4))
        native.check(lib.adk_voc_conv(_p(xg), _p(wf), _p(bg), _p(rg), _p(y), n, cin, t, cout, k, d, G, act, fa, impl, st), "conv")
        native.check(lib.adk_voc_conv_grad(_p(dyg), _p(xa), _p(wb), _p(drg), _p(dx), n, cin, t, cout, k, d, G, act, fa, st), "grad")
        native.check(lib.adk_voc_conv_wgrad(_p(dyg), _p(xg), _p(dw), _p(db), _p(ws), n, cin, t, cout, k, d, G, act, fa, st), "wgrad")
    else:
        assert G == 1
        nb, _ = EG.wgrad_plan(n, cin, t, cout, k, d, 1)
        ws = _nan(gpu, max(1, nb // 4))
        native.check(lib.adk_dec_conv(_p(xg), _p(wf), _p(bg), _p(rg), _p(y), n, cin, t, cout, k, d, act, fa, impl, st), "conv")
        native.check(lib.adk_dec_conv_grad(_p(dyg), _p(xa), _p(wb), _p(drg), _p(dx), n, cin, t, cout, k, d, act, fa, st), "grad")
        native.check(lib.adk_conv_wgrad(_p(dyg), _p(xg), _p(dw), _p(db), _p(ws), n, cin, t, cout, k, d, 1, act, fa, st), "wgrad")
    return y, dx, dw, db


def _convtr_calls(gpu, x, w, b, dy, s, act, alpha, want_db=True, voc=True):
    """adk_voc_convtr, adk_voc_convtr_grad, adk_voc_convtr_wgrad (or the existing three) -> (y, dx, dw, db)."""
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import decoder_train as DT
    lib, native = _lib()
    n, cin, t = x.shape
    cout, k = w.shape[1], 2 * s
    xg, wg_, bg, dyg = (a.to(gpu).contiguous() if a is not None else None for a in (x, w, b, dy))
    wf, wb = DG.pack_convtr(wg_, s), DG.pack_convtr_grad(wg_, s)
    y, dx, dw = _nan(gpu, n, cout, t * s), _nan(gpu, n, cin, t), _nan(gpu, *w.shape)
    db = _nan(gpu, cout) if want_db else None
    nb, _ = DT.convtr_wgrad_plan(n, cin, t, cout, k, s)
    ws = _nan(gpu, nb // 4 + 2)
    st, fa = native.current_stream(gpu), C.c_float(alpha)
    xa = xg if act != NONE else None
    fwd, grad, wgrad = (lib.adk_voc_convtr, lib.adk_voc_convtr_grad, lib.adk_voc_convtr_wgrad) if voc else \
        (lib.adk_dec_convtr, lib.adk_dec_convtr_grad, lib.adk_convtr_wgrad)
    native.check(fwd(_p(xg), _p(wf), _p(bg), _p(y), n, cin, t, cout, k, s, act, fa, st), "convtr")
    native.check(grad(_p(dyg), _p(xa), _p(wb), _p(dx), n, cin, t, cout, k, s, act, fa, st), "convtr_grad")
    native.check(wgrad(_p(dyg), _p(xg), _p(dw), _p(db), _p(ws), n, cin, t, cout, k, s, act, fa, st), "convtr_wgrad")
    return y, dx, dw, db


def _equal(got, ref, what):
    for name, g, r in zip(("y", "dx", "dw", "db"), got, ref):
        if g is None:
            continue
        assert g.shape == r.shape and g.dtype == torch.float32, (what, name)
        assert torch.equal(g.cpu(), r.float()), f"{what} {name}: max diff {float((g.cpu() - r.float()).abs().max())}"


# ---- A. op level, exact ----
# (k, dilation): at k 11 with d 5 the reach is 50, so every T below 51 is all padding edge
KD = [(3, 1), (7, 3), (11, 5), (11, 1), (3, 5)]
TS = [1, 2, 31, 32, 33, 51]


def _exact_conv(gpu, G, cin_g, cout_g, k, d, n, T, slope, options, impl=GEMM):
    cin, cout = G * cin_g, G * cout_g
    rng = np.random.default_rng(10000 * G + 1000 * k + 100 * d + 10 * n + T + cin + cout)
    x, w, dy = _ints(rng, -4, 4, (n, cin, T)), _ints(rng, -3, 3, (cout, cin_g, k)), _ints(rng, -3, 3, (n, cout, T))
    b = _ints(rng, -5, 5, (cout,)) if options & 1 else None
    res = _ints(rng, -5, 5, (n, cout, T)) if options & 2 else None
    dres = _ints(rng, -5, 5, (n, cin, T)) if options & 2 else None
    act = LEAKY if options & 4 else NONE
    ref = _ref_all(lambda a, ww, bb: _conv_ref(a, ww, bb, res.double() if res is not None else None, k, d, G, act, slope),
                   x, w, b, dy, dres, torch.float64)
    got = _conv_calls(gpu, x, w, b, res, dy, dres, k, d, G, act, slope, impl, want_db=bool(options & 8))
    what = f"G{G} ({cin_g},{cout_g}) k{k} d{d} B{n} T{T} slope {slope} options {options:04b} impl {impl}"
    _equal(got, ref, what)
    assert float(ref[0].abs().max()) > 0 and float(ref[2].abs().max()) > 0, what


@pytest.mark.parametrize("G,cin_g,cout_g", [(3, 5, 5), (3, 33, 33), (3, 32, 32), (3, 7, 12), (1, 64, 32)])
def test_conv_exact(gpu, G, cin_g, cout_g):
    """(5, 5): three groups inside one 32-row tile, whose neighbours' rows must be neither read nor written; (33, 33): a group
    straddles a tile; (32, 32): groups end on the tile; (7, 12): rows and columns differ."""
    i = 0
    for k, d in KD:
        for T in TS:
            _exact_conv(gpu, G, cin_g, cout_g, k, d, 1 + 2 * (i % 2), T, (0.5, 0.25)[i // 2 % 2], options=(5 * i + 3) % 16)
            i += 1
    for options in range(16):                                   # every combination of bias, res / dres, the activation and db
        _exact_conv(gpu, G, cin_g, cout_g, 11, 3, 3, 33, 0.25, options)


@pytest.mark.parametrize("cout", [1, 2])
def test_direct_exact(gpu, cout):
    for i, T in enumerate(TS):
        _exact_conv(gpu, 1, 32, cout, 7, 1, 1 + 2 * (i % 2), T, 0.5, options=15 - (i % 4), impl=DIRECT)


def _exact_convtr(gpu, cin, cout, s, n, T, slope, options):
    rng = np.random.default_rng(1000 * s + 100 * n + T + cin + cout)
    x, w, dy = _ints(rng, -4, 4, (n, cin, T)), _ints(rng, -3, 3, (cin, cout, 2 * s)), _ints(rng, -3, 3, (n, cout, T * s))
    b = _ints(rng, -5, 5, (cout,)) if options & 1 else None
    act = LEAKY if options & 4 else NONE
    ref = _ref_all(lambda a, ww, bb: _convtr_ref(a, ww, bb, s, act, slope), x, w, b, dy, None, torch.float64)
    got = _convtr_calls(gpu, x, w, b, dy, s, act, slope, want_db=bool(options & 8))
    _equal(got, ref, f"convtr ({cin},{cout}) s{s} B{n} T{T} slope {slope} options {options:04b}")


@pytest.mark.parametrize("chans", [(64, 32), (33, 5)])
@pytest.mark.parametrize("s", [3, 4, 5])
def test_convtr_exact(gpu, s, chans):
    for i, T in enumerate((1, 2, 3, 33)):
        for n in (1, 3):
            _exact_convtr(gpu, chans[0], chans[1], s, n, T, (0.5, 0.25)[i % 2], options=(4, 13, 5, 12)[(i + n) % 4])


def test_conv_wgrad_exact_split(gpu):
    """groups 3 with S > 1, slices that cut through items and a reduction that ends inside a step: 1050 terms of magnitude <= 12."""
    from audiodec_amd import vocoder_train as VT
    n, T, G, k = 3, 350, 3, 3
    _, S = VT.conv_wgrad_plan(n, 15, T, 15, k, 1, G)
    steps = -(-n * T // 32)
    assert S >= 3 and (n * T) % 32 and steps % S
    _exact_conv(gpu, G, 5, 5, k, 1, n, T, 0.5, options=15)
    _exact_conv(gpu, G, 5, 5, k, 1, n, T, 0.25, options=4)


def test_no_items(gpu):
    lib, native = _lib()
    from audiodec_amd import decoder_train as DT
    from audiodec_amd import vocoder_train as VT
    st, fa = native.current_stream(gpu), C.c_float(0.1)
    e = torch.empty(0, device=gpu)
    keep = _nan(gpu, 4)
    assert lib.adk_voc_conv(_p(e), _p(keep), None, None, _p(keep), 0, 6, 5, 6, 3, 1, 3, LEAKY, fa, GEMM, st) == 0
    assert lib.adk_voc_conv_grad(_p(e), _p(e), _p(keep), None, _p(keep), 0, 6, 5, 6, 3, 1, 3, LEAKY, fa, st) == 0
    assert lib.adk_voc_convtr(_p(e), _p(keep), None, _p(keep), 0, 6, 5, 4, 6, 3, LEAKY, fa, st) == 0
    assert lib.adk_voc_convtr_grad(_p(e), _p(e), _p(keep), _p(keep), 0, 6, 5, 4, 6, 3, LEAKY, fa, st) == 0
    assert bool(torch.isnan(keep).all())                        # forward and backward: nothing is written
    dw, db = _nan(gpu, 6, 2, 3), _nan(gpu, 6)
    ws = _nan(gpu, max(1, VT.conv_wgrad_plan(0, 6, 5, 6, 3, 1, 3)[0] // 4))
    assert lib.adk_voc_conv_wgrad(None, None, _p(dw), _p(db), _p(ws), 0, 6, 5, 6, 3, 1, 3, LEAKY, fa, st) == 0
    assert not dw.any() and not db.any()                        # the weight gradients: zeros
    dw, db = _nan(gpu, 6, 4, 6), _nan(gpu, 4)
    ws = _nan(gpu, DT.convtr_wgrad_plan(0, 6, 5, 4, 6, 3)[0] // 4 + 2)
    assert lib.adk_voc_convtr_wgrad(None, None, _p(dw), _p(db), _p(ws), 0, 6, 5, 4, 6, 3, LEAKY, fa, st) == 0
    assert not dw.any() and not db.any()


# ---- B. group isolation ----
@pytest.mark.parametrize("cin_g,cout_g", [(5, 5), (33, 33), (7, 12)])
def test_group_isolation(gpu, cin_g, cout_g):
    G, k, d, n, T = 3, 11, 3, 2, 40
    rng = np.random.default_rng(cin_g + cout_g)
    x, w, b = _real(rng, (n, G * cin_g, T)), _real(rng, (G * cout_g, cin_g, k)), _real(rng, (G * cout_g,))
    dy, res, dres = _real(rng, (n, G * cout_g, T)), _real(rng, (n, G * cout_g, T)), _real(rng, (n, G * cin_g, T))
    clean = _conv_calls(gpu, x, w, b, res, dy, dres, k, d, G, LEAKY, 0.1)
    xs, ys = slice(cin_g, 2 * cin_g), slice(cout_g, 2 * cout_g)
    xn, dyn = x.clone(), dy.clone()
    xn[:, xs] = float("nan")
    dyn[:, ys] = float("nan")
    for xx, dd in ((xn, dy), (x, dyn), (xn, dyn)):
        y, dx, dw, db = _conv_calls(gpu, xx, w, b, res, dd, dres, k, d, G, LEAKY, 0.1)
        for g in (0, 2):
            rows, chans = slice(g * cout_g, (g + 1) * cout_g), slice(g * cin_g, (g + 1) * cin_g)
            for got, ref in ((y[:, rows], clean[0][:, rows]), (dx[:, chans], clean[1][:, chans]), (dw[rows], clean[2][rows]),
                             (db[rows], clean[3][rows])):
                assert bool(torch.isfinite(got).all()) and torch.equal(got, ref)
        if xx is xn:
            assert bool(torch.isnan(y[:, ys]).all()) and bool(torch.isnan(dw[ys]).all())        # the NaN did arrive where it belongs
        if dd is dyn:
            assert bool(torch.isnan(dx[:, xs]).all()) and bool(torch.isnan(db[ys]).all())


# ---- C. equivalence with the existing entry points ----
@pytest.mark.parametrize("act", [NONE, ELU])
def test_one_group_equals_existing_calls(gpu, act):
    rng = np.random.default_rng(40 + act)
    for cin, cout, k, d, n, T in ((64, 32, 7, 3, 2, 50), (33, 136, 7, 9, 3, 33), (256, 256, 1, 1, 1, 40)):
        x, w, b = _real(rng, (n, cin, T), 1.5), _real(rng, (cout, cin, k)), _real(rng, (cout,))
        dy, res, dres = _real(rng, (n, cout, T)), _real(rng, (n, cout, T)), _real(rng, (n, cin, T))
        new = _conv_calls(gpu, x, w, b, res, dy, dres, k, d, 1, act, 0.7)
        old = _conv_calls(gpu, x, w, b, res, dy, dres, k, d, 1, act, 0.7, voc=False)
        assert all(torch.equal(a, o) for a, o in zip(new, old)), (cin, cout, k)
    x, w, b, dy = _real(rng, (2, 32, 33), 1.5), _real(rng, (1, 32, 7)), _real(rng, (1,)), _real(rng, (2, 1, 33))
    new = _conv_calls(gpu, x, w, b, None, dy, None, 7, 1, 1, act, 0.7, impl=DIRECT)
    old = _conv_calls(gpu, x, w, b, None, dy, None, 7, 1, 1, act, 0.7, impl=DIRECT, voc=False)
    assert all(torch.equal(a, o) for a, o in zip(new, old))
    for cin, cout, s, n, T in ((64, 32, 3, 2, 33), (136, 128, 5, 3, 7), (33, 5, 4, 1, 1)):
        x, w, b, dy = _real(rng, (n, cin, T), 1.5), _real(rng, (cin, cout, 2 * s)), _real(rng, (cout,)), _real(rng, (n, cout, T * s))
        new = _convtr_calls(gpu, x, w, b, dy, s, act, 0.7)
        old = _convtr_calls(gpu, x, w, b, dy, s, act, 0.7, voc=False)
        assert all(torch.equal(a, o) for a, o in zip(new, old)), (cin, cout, s)


# ---- D. real values and real slopes ----
def _bounded(got, ref64, ref32, what):
    """max|got - ref64| <= 4 E + 1e-6 max|ref64|, E = max|ref32 - ref64| (torch's f32 on the CPU)."""
    e, m = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
    err = float((got.cpu().double() - ref64).abs().max())
    bound = 4 * e + 1e-6 * m
    print(f"{what}: err {err:.3e} E {e:.3e} max {m:.3f} err/bound {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("slope", [0.1, 0.01])
@pytest.mark.parametrize("G,cin_g,cout_g,k,d,n,T", [(3, 32, 32, 11, 5, 2, 96), (3, 64, 64, 3, 1, 2, 40), (3, 33, 33, 11, 3, 3, 33),
                                                    (1, 128, 128, 7, 3, 2, 64), (1, 96, 32, 1, 1, 2, 50)])
def test_conv_real_values(gpu, G, cin_g, cout_g, k, d, n, T, slope):
    rng = np.random.default_rng(7 + G + cin_g + k + d + T)
    x, w, b = _real(rng, (n, G * cin_g, T), 1.5), _real(rng, (G * cout_g, cin_g, k), 0.1), _real(rng, (G * cout_g,))
    assert float((x < 0).float().mean()) > 0.3
    dy, res, dres = _real(rng, (n, G * cout_g, T)), _real(rng, (n, G * cout_g, T)), _real(rng, (n, G * cin_g, T))
    fwd = lambda dt: (lambda a, ww, bb: _conv_ref(a, ww, bb, res.to(dt), k, d, G, LEAKY, slope))          # noqa: E731
    r64 = _ref_all(fwd(torch.float64), x, w, b, dy, dres, torch.float64)
    r32 = _ref_all(fwd(torch.float32), x, w, b, dy, dres, torch.float32)
    got = _conv_calls(gpu, x, w, b, res, dy, dres, k, d, G, LEAKY, slope)
    for name, g, a, c in zip(("y", "dx", "dW", "db"), got, r64, r32):
        _bounded(g, a, c, f"conv G{G} ({cin_g},{cout_g}) k{k} d{d} slope {slope} {name}")


@pytest.mark.parametrize("slope", [0.1, 0.01])
@pytest.mark.parametrize("s,T,n,cin,cout", [(3, 33, 2, 64, 32), (5, 26, 3, 256, 128), (4, 1, 3, 40, 7)])
def test_convtr_real_values(gpu, s, T, n, cin, cout, slope):
    rng = np.random.default_rng(7 + s + T + n + cin + cout)
    x, w, b = _real(rng, (n, cin, T), 1.5), _real(rng, (cin, cout, 2 * s), 0.1), _real(rng, (cout,))
    dy = _real(rng, (n, cout, T * s))
    fwd = lambda a, ww, bb: _convtr_ref(a, ww, bb, s, LEAKY, slope)                                     # noqa: E731
    r64, r32 = _ref_all(fwd, x, w, b, dy, None, torch.float64), _ref_all(fwd, x, w, b, dy, None, torch.float32)
    got = _convtr_calls(gpu, x, w, b, dy, s, LEAKY, slope)
    for name, g, a, c in zip(("y", "dx", "dW", "db"), got, r64, r32):
        _bounded(g, a, c, f"convtr s{s} T{T} ({cin},{cout}) slope {slope} {name}")


# ---- E. whole vocoder ----
def _vocoder(gpu, name):
    from audiodec_amd import vocoder_train as VT
    tag, p = MVG.generator_params(name)
    voc = VT.TrainableVocoder(**p)
    voc.load_state_dict(synth.synth_state_dict(tag, MFG.SEED))
    return voc.to(gpu)


def _stream_generator(gpu, name, sd, streams, frames):
    from audiodec_amd.stream_generator import HiFiGANStreamGenerator
    _, p = MVG.generator_params(name)
    gen = HiFiGANStreamGenerator(**p)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen.load_state_dict(sd)
    gen = gen.eval().to(gpu)
    gen.set_offline(True)
    gen.configure(num_streams=streams, max_frames=frames)
    return gen


@pytest.mark.parametrize("name,n_params", [("v1", 98), ("v0", 234), ("noaddl", 62)])
def test_vocoder_against_reference(gpu, golden_dir, name, n_params):
    fx = np.load(os.path.join(golden_dir, f"vocoder_train_{name}.npz"), allow_pickle=False)
    voc = _vocoder(gpu, name)
    c = torch.from_numpy(MVG.case_input()).to(gpu).requires_grad_(True)
    y = voc(c)
    y64 = fx["y64"]
    assert tuple(y.shape) == y64.shape and y.requires_grad
    y.backward(torch.from_numpy(MVG.upstream(int(fx["seed"]), y64.shape)).to(gpu))
    names = [str(k) for k in fx["names"]]
    params = dict(voc.named_parameters())
    assert set(params) == set(names) and len(names) == n_params
    got = [y.detach().cpu().numpy().reshape(-1), c.grad.cpu().numpy().reshape(-1)] + \
          [MVG.sample(params[k].grad.cpu().numpy()) for k in names]
    ref = [y64.reshape(-1), fx["gc64"].reshape(-1)] + [fx[f"g{i}"] for i in range(len(names))]
    worst, where = 0.0, ""
    for what, g, r, e, m in zip(["y", "c"] + names, got, ref, fx["E_ref"], fx["max"]):
        assert g.shape == r.shape, what
        err, bound = float(np.abs(g.astype(np.float64) - r).max()), 4 * float(e) + 1e-6 * float(m)
        if err / bound > worst:
            worst, where = err / bound, what
        assert err <= bound, f"{name} {what}: {err:.3e} > {bound:.3e}"
    print(f"vocoder {name}: largest err/bound {worst:.3f} ({where})")
    assert voc.saved_floats(2, 7) > 0


@pytest.mark.parametrize("name", ["v1", "v0", "noaddl"])
def test_against_the_inference_path(gpu, name):
    tag, _ = MVG.generator_params(name)
    sd = synth.synth_state_dict(tag, MFG.SEED)
    voc = _vocoder(gpu, name)
    c = torch.from_numpy(MVG.case_input()).to(gpu)
    with torch.no_grad():
        y = voc(c)
        assert not y.requires_grad and y.grad_fn is None
        gen = _stream_generator(gpu, name, sd, 2, 7)
        ys = torch.as_tensor(gen.decode(c.transpose(1, 2).contiguous())).clone()
    err = float((ys - y).abs().max())
    print(f"{name}: TrainableVocoder vs the offline program {err:.3e} (bound {WAVE_TOL})")
    assert ys.shape == y.shape == (2, 1, 2100) and err <= WAVE_TOL


# ---- F. reproducibility, accumulation, the stage-2 step, behaviour ----
@pytest.mark.parametrize("name", ["v1", "v0"])
def test_reproducible_and_accumulates(gpu, name):
    voc = _vocoder(gpu, name)
    c_np = MVG.case_input()
    up = torch.from_numpy(MVG.upstream(5, (2, 1, 2100))).to(gpu)
    with torch.no_grad():
        y0 = voc(torch.from_numpy(c_np).to(gpu))
    runs = []
    for _ in range(2):
        voc.zero_grad(set_to_none=True)
        c = torch.from_numpy(c_np).to(gpu).requires_grad_(True)
        y = voc(c)
        y.backward(up)
        runs.append([y.detach().clone(), c.grad.clone()] + [p.grad.clone() for p in voc.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(runs[0][0], y0)                          # with and without the graph: the same forward
    y = voc(torch.from_numpy(c_np).to(gpu))
    assert y.requires_grad                                      # the parameters ask for the graph
    y.backward(up)
    assert all(torch.equal(p.grad, g + g) for p, g in zip(voc.parameters(), runs[0][2:]))      # g + g is exact


class _Counter:
    """Counts the calls of one native entry point through a wrapper on the loaded library object."""

    def __init__(self, name):
        from audiodec_amd import native
        self.lib, self.name, self.calls = native.lib(), name, 0
        self.orig = getattr(self.lib, name)

    def __enter__(self):
        def wrapped(*a):
            self.calls += 1
            return self.orig(*a)
        setattr(self.lib, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)


def _waves(seed, B, n):
    return torch.from_numpy(np.stack([synth.synth_audio(seed, s, n) for s in range(B)]))[:, None, :]


def test_stage2_step(gpu):
    """trainer/vocoder.py:65-90: the analyzer frozen, the vocoder learns from mel(voc(zq), x) plus the generator's adversarial loss,
    which reaches y_ through the HiFi-GAN discriminator's backward to its input."""
    from audiodec_amd import decoder_grad as DG
    from audiodec_amd import discriminator as D
    from audiodec_amd import encoder_grad as EG
    from audiodec_amd import mel
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    enc_tag, pe = MTG.generator_params("vctk_sym")
    analyzer = AutoEncoderStreamGenerator(**pe)
    analyzer.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    analyzer = analyzer.eval().to(gpu)
    enc = EG.TrainableEncoder.from_generator(analyzer)
    for p in enc.parameters():
        p.requires_grad_(False)
    tag, _ = MVG.generator_params("v1")
    sd = synth.synth_state_dict(tag, MFG.SEED)
    voc = _vocoder(gpu, "v1")
    loss = mel.MultiMelSpectrogramLoss(fs=48000, device=gpu, differentiable=True)
    disc = D.Discriminator(**DO.PARAMS["reduced"], device=gpu, differentiable=True).load_state_dict(DO.state_dict("reduced"))
    adv = D.GeneratorAdversarialLoss(False, "mse", differentiable=True)
    B, frames = 2, 4                                            # the mel loss's largest FFT needs more than 1024 samples
    x = _waves(17, B, frames * 300).to(gpu)
    params = list(voc.parameters())
    runs = []
    for _ in range(2):
        voc.zero_grad(set_to_none=True)
        with _Counter("adk_conv_wgrad") as cw, _Counter("adk_enc_down_grad") as eg, _Counter("adk_voc_conv_wgrad") as vw, \
                _Counter("adk_voc_convtr_wgrad") as tw, _Counter("adk_voc_conv_grad") as vg:
            zq, _, _ = DG.quantize_st(analyzer, enc(x))
            assert not zq.requires_grad
            y_ = voc(zq)
            total = loss(y_, x) + adv(disc(y_))
            total.backward()
        # the vocoder's 30 stride-1 and 4 transposed convs; zq is a constant, so input_conv's dx is not computed; no encoder launch
        assert (cw.calls, eg.calls, vw.calls, tw.calls, vg.calls) == (0, 0, 30, 4, 29)
        runs.append([total.detach().clone()] + [p.grad.clone() for p in params])
    assert len(params) == 98 and all(g.shape == p.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
                                     for g, p in zip(runs[0][1:], params))
    assert all(torch.equal(a, b) for a, b in zip(*runs))        # bitwise the first run
    assert all(p.grad is None for p in enc.parameters())
    before = [p.detach().clone() for p in params]
    torch.optim.Adam(params, lr=1e-4).step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    with torch.no_grad():
        zq3 = zq[:, :, :3].contiguous()
        y3 = voc(zq3)
        assert not torch.equal(y3, _vocoder(gpu, "v1")(zq3))   # the packings followed the parameters
    gen = _stream_generator(gpu, "v1", {**sd, **voc.state_dict()}, B, 3)
    with torch.no_grad():
        y_stream = torch.as_tensor(gen.decode(zq3.transpose(1, 2).contiguous())).clone()
    err = float((y_stream - y3).abs().max())
    print(f"stage 2: the generator's decode of the trained weights vs TrainableVocoder {err:.3e} (bound {WAVE_TOL})")
    assert y_stream.shape == y3.shape == (B, 1, 900) and err <= WAVE_TOL


def test_launch_counts_and_second_backward(gpu):
    voc = _vocoder(gpu, "noaddl")
    c = torch.from_numpy(MVG.case_input()[:, :, :2]).to(gpu)
    up = torch.from_numpy(MVG.upstream(3, (2, 1, 600))).to(gpu)
    names = ("adk_voc_conv_wgrad", "adk_voc_convtr_wgrad", "adk_voc_conv_grad", "adk_voc_convtr_grad")

    def counted(fn):
        with _Counter(names[0]) as a, _Counter(names[1]) as b, _Counter(names[2]) as c_, _Counter(names[3]) as d:
            fn()
        return a.calls, b.calls, c_.calls, d.calls

    y = voc(c)
    # 18 stride-1 convs (input, 4 x 3 units, 4 conv_out, output) and 4 transposed; c is a constant: input_conv's dx is not computed
    assert counted(lambda: y.backward(up)) == (18, 4, 17, 4) and c.grad is None
    full = {k: p.grad.clone() for k, p in voc.named_parameters()}
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        y.backward(up)
    voc.zero_grad(set_to_none=True)
    cg = c.clone().requires_grad_(True)
    assert counted(lambda: voc(cg).backward(up)) == (18, 4, 18, 4) and float(cg.grad.abs().max()) > 0
    assert all(torch.equal(p.grad, full[k]) for k, p in voc.named_parameters())
    # frozen parameters: no gradient, and a weight-gradient launch only where a weight or a bias still asks for one
    voc.zero_grad(set_to_none=True)
    frozen = ["blocks.1.convs1.2.conv.weight_g", "blocks.1.convs1.2.conv.weight_v", "blocks.1.convs1.2.conv.bias",      # a whole conv
              "upsamples.2.deconv.weight_g", "upsamples.2.deconv.weight_v",                                            # its bias remains
              "upsamples.3.deconv.weight_g", "upsamples.3.deconv.weight_v", "upsamples.3.deconv.bias",
              "blocks.0.conv_out.weight_g"]                                                                            # weight_v remains
    for k in frozen:
        voc.get_parameter(k).requires_grad_(False)
    assert counted(lambda: voc(c).backward(up))[:2] == (17, 3)
    for k, p in voc.named_parameters():
        assert (p.grad is None) if k in frozen else torch.equal(p.grad, full[k]), k
    for p in voc.parameters():
        p.requires_grad_(False)
    assert not voc(c).requires_grad                             # nothing asks for a gradient: no graph
    voc.zero_grad(set_to_none=True)
    cg2 = c.clone().requires_grad_(True)
    assert counted(lambda: voc(cg2).backward(up)) == (0, 0, 18, 4) and all(p.grad is None for p in voc.parameters())
    assert torch.equal(cg2.grad, cg.grad)                       # the backward to the input does not depend on who is trainable


def test_without_weight_norm(gpu):
    """use_weight_norm=False: the same network on plain `weight` parameters.  Loaded with the composed weights of the weight-normed
    module it gives the same output bit for bit, and its weight gradients are the dW that the other module passes on to g and v."""
    from audiodec_amd import vocoder_train as VT
    _, p = MVG.generator_params("noaddl")
    wn = _vocoder(gpu, "noaddl")
    plain = VT.TrainableVocoder(**{**p, "use_weight_norm": False}).to(gpu)
    sd = {k: v for k, v in wn.state_dict().items() if not k.endswith(("weight_g", "weight_v"))}
    for s in wn._specs:
        sd[s.wkey("weight")] = VT.weight_norm(wn.get_parameter(s.wkey("weight_g")), wn.get_parameter(s.wkey("weight_v"))).detach()
    plain.load_state_dict(sd)
    c = torch.from_numpy(MVG.case_input()).to(gpu)
    up = torch.from_numpy(MVG.upstream(5, (2, 1, 2100))).to(gpu)
    y, yp = wn(c), plain(c)
    assert torch.equal(y, yp)
    y.backward(up)
    yp.backward(up)
    for s in wn._specs:
        g, v, w = (m.get_parameter(s.wkey(k)) for m, k in ((wn, "weight_g"), (wn, "weight_v"), (plain, "weight")))
        assert w.grad.shape == w.shape and bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0
        gr, vr = g.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
        VT.weight_norm(gr, vr).backward(w.grad)                  # the composition's own backward, fed the plain module's dW
        assert torch.equal(gr.grad, g.grad) and torch.equal(vr.grad, v.grad), s.name
        if s.bias:
            assert torch.equal(plain.get_parameter(s.wkey("bias")).grad, wn.get_parameter(s.wkey("bias")).grad)


def test_from_generator_on_device(gpu):
    from audiodec_amd import vocoder_train as VT
    tag, _ = MVG.generator_params("noaddl")
    gen = _stream_generator(gpu, "noaddl", synth.synth_state_dict(tag, MFG.SEED), 2, 7)
    voc = VT.TrainableVocoder.from_generator(gen)
    assert next(voc.parameters()).device == torch.device(gpu) and voc.mean.device == torch.device(gpu)
    c = torch.from_numpy(MVG.case_input()).to(gpu)
    with torch.no_grad():
        assert torch.equal(voc(c), _vocoder(gpu, "noaddl")(c))
