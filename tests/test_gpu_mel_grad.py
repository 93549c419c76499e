"""GPU: the mel-spectrogram loss's backward (adk_logmel_vjp, adk_mel_distance_grad) against the fp64 restatement.

  A. every case and resolution of mel_grad_oracle.CASES: the VJP of a standard-normal upstream gradient within
     ||hip - fp64|| <= 4 relerr32 ||fp64|| + 1e-6 ||fp64||, relerr32 being the reference's own float32 error (mel_grad.npz);
  B. the loss gradient: the sign of logmel(y_hat) - logmel(y) is discontinuous, so the HIP sign pattern (from the HIP log-mels,
     which are the very values the backward recomputes) must equal the fp64 one except where fp64 |difference| < 1e-4, those
     being at most 1 % of the elements; the gradient is then held to the fp64 gradient computed WITH the HIP signs, within A's bound;
  C. the value is the non-differentiable object's; bitwise reproducibility; exact power-of-two linearity in the upstream factor;
     2-D and 3-D layouts; silence; uncovered samples; NaN input; one SGD step lowers the loss.
"""
import os

import numpy as np
import pytest
import torch

import mel_grad_oracle as GO
import mel_oracle as MO

pytestmark = pytest.mark.gpu

IDS = [GO.key(*c) for c in GO.CASES]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "mel_grad.npz"), allow_pickle=False)


def _loss(pname, gpu, differentiable=True):
    from audiodec_amd import mel
    return mel.MultiMelSpectrogramLoss(**GO.params(pname), device=gpu, differentiable=differentiable)


def _leaf(a, gpu):
    return torch.from_numpy(a).to(gpu).requires_grad_(True)


def _grad(loss, y_hat, y, gpu, factor=None):
    a = _leaf(y_hat, gpu)
    v = loss(a, torch.from_numpy(y).to(gpu))
    (v if factor is None else factor * v).backward()
    return v.detach(), a.grad


def _bound(relerr32, exact):
    return (4 * relerr32 + 1e-6) * float(np.linalg.norm(exact.ravel()))


@pytest.mark.parametrize("pname,shape", GO.CASES, ids=IDS)
def test_vjp_against_fp64(gpu, fixture, pname, shape):
    p, K = GO.params(pname), GO.key(pname, shape)
    loss = _loss(pname, gpu)
    mms = GO.melmats(p)
    y_hat, _ = GO.inputs(shape)
    n = int(np.prod(shape[:-1]))
    for r, (f, (n_fft, hop, wl)) in enumerate(zip(loss.mel_transfers, MO.resolutions(p))):
        g = GO.upstream(pname, shape, r, p)
        a = _leaf(y_hat, gpu)
        lm = f(a)
        assert tuple(lm.shape) == g.shape and lm.requires_grad
        lm.backward(torch.from_numpy(g).to(gpu))
        assert a.grad.shape == a.shape and a.grad.dtype == torch.float32
        got = a.grad.reshape(n, -1).cpu().numpy().astype(np.float64)
        exact = GO.vjp64(y_hat, g, n_fft, hop, wl, mms[r], p["eps"], p["log_base"])
        err, rel32 = float(np.linalg.norm((got - exact).ravel())), float(fixture[f"{K}_relerr32_vjp{r}"])
        bound = _bound(rel32, exact)
        print(f"{K} r{r}: VJP relerr hip {err / np.linalg.norm(exact.ravel()):.3g} ref32 {rel32:.3g} ratio to bound {err / bound:.3f}")
        assert err <= bound, f"{K} r{r}: ||hip - fp64|| {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("pname,shape", GO.CASES, ids=IDS)
def test_loss_gradient_against_fp64_with_hip_signs(gpu, fixture, pname, shape):
    p, K = GO.params(pname), GO.key(pname, shape)
    loss = _loss(pname, gpu)
    mms = GO.melmats(p)
    y_hat, y = GO.inputs(shape)
    n = int(np.prod(shape[:-1]))
    signs, fragile, total = [], 0, 0
    with torch.no_grad():
        for f, (s64, d64) in zip(loss.mel_transfers, GO.signs64(y_hat, y, p, mms)):
            la, lb = f(torch.from_numpy(y_hat).to(gpu)), f(torch.from_numpy(y).to(gpu))
            s_hip = torch.sign(la - lb).cpu().numpy().astype(np.float64)
            weak = d64 < 1e-4
            assert np.array_equal(s_hip[~weak], s64[~weak]), f"{K}: a sign differs where fp64 |lm_a - lm_b| >= 1e-4"
            fragile, total = fragile + int(weak.sum()), total + weak.size
            signs.append(s_hip)
    assert fragile <= 0.01 * total, f"{K}: {fragile} of {total} elements are fragile"
    _, grad = _grad(loss, y_hat, y, gpu)
    assert grad.shape == tuple(shape) and grad.dtype == torch.float32
    got = grad.reshape(n, -1).cpu().numpy().astype(np.float64)
    exact = GO.loss_grad64(y_hat, y, p, mms, signs=signs)
    rel32 = max(float(fixture[f"{K}_relerr32_vjp{r}"]) for r in range(len(mms)))
    err, bound = float(np.linalg.norm((got - exact).ravel())), _bound(rel32, exact)
    print(f"{K}: loss gradient relerr hip {err / np.linalg.norm(exact.ravel()):.3g} ref32 {rel32:.3g} ratio to bound "
          f"{err / bound:.3f} fragile {fragile}/{total}")
    assert err <= bound, f"{K}: ||hip - fp64|| {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("pname,shape", [("defaults", (2, 1, 7777)), ("small", (8, 1, 9600))])
def test_value_reproducibility_and_linearity(gpu, pname, shape):
    y_hat, y = GO.inputs(shape)
    loss = _loss(pname, gpu)
    v1, g1 = _grad(loss, y_hat, y, gpu)
    v2, g2 = _grad(loss, y_hat, y, gpu)
    with torch.no_grad():
        plain = _loss(pname, gpu, differentiable=False)(torch.from_numpy(y_hat).to(gpu), torch.from_numpy(y).to(gpu))
        quiet = loss(_leaf(y_hat, gpu), torch.from_numpy(y).to(gpu))
    assert v1.dim() == 0 and v1.dtype == torch.float32
    assert torch.equal(v1, plain) and torch.equal(quiet, plain) and not quiet.requires_grad
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0 and torch.isfinite(g1).all()
    _, g4 = _grad(loss, y_hat, y, gpu, factor=4.0)
    assert torch.equal(g4, 4 * g1)
    f = loss.mel_transfers[0]
    up = torch.from_numpy(GO.upstream(pname, shape, 0, GO.params(pname))).to(gpu)
    vj = []
    for _ in range(2):
        a = _leaf(y_hat, gpu)
        f(a).backward(up)
        vj.append(a.grad)
    assert torch.equal(vj[0], vj[1])
    # a tensor that does not require grad, on a differentiable object: today's behaviour
    lm = f(torch.from_numpy(y).to(gpu))
    assert not lm.requires_grad and torch.equal(lm, _loss(pname, gpu, False).mel_transfers[0](torch.from_numpy(y).to(gpu)))


def test_double_backward_raises(gpu):
    y_hat, y = GO.inputs((1, 1, 1025))
    a = _leaf(y_hat, gpu)
    v = _loss("vctk", gpu)(a, torch.from_numpy(y).to(gpu))
    (g,) = torch.autograd.grad(v, a, create_graph=True)
    assert not g.requires_grad                                   # the gradient is a constant to autograd
    with pytest.raises(RuntimeError, match="does not require grad"):
        g.sum().backward()
    # an upstream gradient that itself requires grad asks for the second derivative: once_differentiable's error
    w = torch.ones((), device=gpu, requires_grad=True)
    a = _leaf(y_hat, gpu)
    (g,) = torch.autograd.grad(_loss("vctk", gpu)(a, torch.from_numpy(y).to(gpu)) * w, a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_layouts_2d_and_3d(gpu):
    y_hat, y = GO.inputs((2, 4500))
    loss = _loss("vctk", gpu)
    _, g2 = _grad(loss, y_hat, y, gpu)
    _, g3 = _grad(loss, y_hat.reshape(2, 1, 4500), y.reshape(2, 1, 4500), gpu)
    assert g2.shape == (2, 4500) and g3.shape == (2, 1, 4500) and torch.equal(g2, g3.reshape(2, 4500))
    a = _leaf(y_hat, gpu).to(torch.float64).detach().requires_grad_(True)          # the gradient takes y_hat's dtype
    loss(a, torch.from_numpy(y).to(gpu)).backward()
    assert a.grad.dtype == torch.float64 and torch.equal(a.grad.float(), g2)


def test_silence_gives_an_exact_zero(gpu):
    _, y = GO.inputs((2, 1, 4800))
    for pname in ("vctk", "defaults"):
        v, g = _grad(_loss(pname, gpu), np.zeros_like(y), y, gpu)
        assert torch.isfinite(v) and torch.isfinite(g).all() and int(torch.count_nonzero(g)) == 0


def test_uncovered_samples_get_an_exact_zero(gpu):
    shape = (2, 1, 2000)
    y_hat, y = GO.inputs(shape)
    _, g = _grad(_loss("gap", gpu), y_hat, y, gpu)
    bare = GO.coverage(2000, 256, 300, 256) == 0
    zero = (g.reshape(2, 2000) == 0).cpu().numpy()
    assert int(bare.sum()) * 2 == 684
    assert np.array_equal(zero, np.broadcast_to(bare, zero.shape))
    a = _leaf(y_hat, gpu)                                                         # the VJP shares the overlap-add
    _loss("gap", gpu).mel_transfers[0](a).backward(torch.ones(2, 40, 7, device=gpu))
    assert np.array_equal((a.grad.reshape(2, 2000) == 0).cpu().numpy(), zero)


def test_nan_input_raises_no_flag(gpu):
    from audiodec_amd import native
    y_hat, y = GO.inputs((2, 4500))
    y_hat = y_hat.copy()
    y_hat[0, 1000] = np.nan
    v, g = _grad(_loss("vctk", gpu), y_hat, y, gpu)
    assert torch.isnan(v) and g.shape == (2, 4500)
    assert torch.isfinite(g[1]).all()                                             # the other signal is untouched by it
    assert native.device_flags() == 0


def test_one_sgd_step_lowers_the_loss(gpu):
    y_hat, y = GO.inputs((3, 1, 9600))
    loss = _loss("vctk", gpu)
    a, b = _leaf(y_hat, gpu), torch.from_numpy(y).to(gpu)
    opt = torch.optim.SGD([a], lr=5e-2)
    v0 = loss(a, b)
    v0.backward()
    opt.step()
    with torch.no_grad():
        v1 = loss(a, b)
    print(f"loss {float(v0):.6f} -> {float(v1):.6f}")
    assert float(v1) < float(v0)
