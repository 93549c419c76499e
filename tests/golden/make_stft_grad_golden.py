#!/usr/bin/env python3
"""Generate tests/golden/stft_grad.npz: the reference's multi-resolution STFT loss (losses/stft_loss.py) and waveform-shape loss
(losses/waveform_loss.py) run backward by autograd.

Runs only where the reference is available.  It imports the UNMODIFIED reference modules the way make_stft_golden.py does and
runs them on the CPU in float32.  Per case ``K`` of stft_grad_oracle.CASES (``K = stft_grad_oracle.key(params, shape)``) and
resolution ``r`` it stores the reference's own float32 relative L2 error against the fp64 oracle EVALUATED WITH THE REFERENCE'S
FLOAT32 SIGNS AND MASKS (sign(log y_mag - log x_mag) and power(x) >= eps are discontinuous: like is compared with like):
  K_relerr32_sc<r>    the gradient of STFTLoss r's spectral-convergence term with respect to x = y_hat
  K_relerr32_mag<r>   the same for its log-magnitude term
  K_relerr32_vjp<r>   stft()'s VJP of stft_grad_oracle.upstream(...) (standard normal, seeded)
  K_weak<r>, K_fragile<r>   elements with fp64 |log y_mag - log x_mag| < 1e-4; with fp64 power(x) in [eps/2, 2 eps]
  K_signdiff<r>, K_maskdiff<r>   elements whose float32 sign / mask differs from the fp64 one
  K_grad_sc, K_grad_mag, K_vjp<r>   the float32 gradients of MultiResolutionSTFTLoss's two outputs and the VJPs themselves, for
                                    cases of at most stft_grad_oracle.STORE_MAX_SAMPLES samples
and per shape case ``S`` (``stft_grad_oracle.shape_key``) ``S_grad``, the float32 gradient of MultiWindowShapeLoss with respect to
y_hat (same size rule; the constructed cases always).  It asserts what the GPU test relies on: weak signs are at most 1 % and
fragile masks at most 8 elements of a resolution; no shape case but the constructed ones has a tied maximum or an equal pair of
maxima; in the constructed tie case the reference gives the first index the gradient.  Change a case's seed if one fails.
Inputs are regenerated from seeds, not stored.  Fixed member times: a rerun on the same software gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import stft_grad_oracle as SG  # noqa: E402
import stft_oracle as SO  # noqa: E402
from make_mel_golden import import_mel_loss  # noqa: E402

OUT = os.path.join(HERE, "stft_grad.npz")


def _leaf(a):
    return torch.from_numpy(a.reshape(-1, a.shape[-1])).clone().requires_grad_(True)


def stft_case(stft_loss, pname, shape, out):
    p, K = SG.params(pname), SG.key(pname, shape)
    y_hat, y = SG.inputs(shape)
    loss = stft_loss.MultiResolutionSTFTLoss(**p)
    yt = torch.from_numpy(y.reshape(-1, y.shape[-1]))
    wins = SG.windows_f32(p)
    line = []
    for r, (f, (n_fft, hop, wl)) in enumerate(zip(loss.stft_losses, SO.resolutions(p))):
        with torch.no_grad():                                            # the reference's float32 signs and masks
            xt = torch.from_numpy(y_hat.reshape(-1, y_hat.shape[-1]))
            spec = torch.stft(xt, n_fft, hop, wl, f.window, return_complex=True)
            mask = ((spec.real ** 2 + spec.imag ** 2) >= SG.EPS).transpose(2, 1).numpy()
            xm, ym = (stft_loss.stft(t, n_fft, hop, wl, f.window) for t in (xt, yt))
            sign = torch.sign(torch.log(ym) - torch.log(xm)).numpy()
        grads = []
        for term in (0, 1):
            a = _leaf(y_hat)
            f(a, yt)[term].backward()
            grads.append(a.grad.numpy().copy())
        exact = [SG.res_grad64(y_hat, y, n_fft, hop, wl, wins[r], 1.0, 0.0, SG.EPS, sign, mask),
                 SG.res_grad64(y_hat, y, n_fft, hop, wl, wins[r], 0.0, 1.0, SG.EPS, sign, mask)]
        g = SG.upstream(pname, shape, r, p)
        a = _leaf(y_hat)
        stft_loss.stft(a, n_fft, hop, wl, f.window).backward(torch.from_numpy(g))
        vjp = a.grad.numpy().copy()
        out[f"{K}_relerr32_sc{r}"] = np.float64(SG.rel_l2(grads[0], exact[0]))
        out[f"{K}_relerr32_mag{r}"] = np.float64(SG.rel_l2(grads[1], exact[1]))
        out[f"{K}_relerr32_vjp{r}"] = np.float64(SG.rel_l2(vjp, SG.mag_vjp64(y_hat, g, n_fft, hop, wl, wins[r], SG.EPS, mask)))
        if SG.stored(shape):
            out[f"{K}_vjp{r}"] = vjp.astype(np.float32)
        dlog = np.abs(SG.dlog64(y_hat, y, p)[r])
        power = SG.power64(y_hat, n_fft, hop, wl, wins[r])
        weak = int((dlog < SG.WEAK_DLOG).sum())
        fragile = int(((power >= SG.EPS / 2) & (power <= 2 * SG.EPS)).sum())
        assert weak <= SG.WEAK_CAP * dlog.size, f"{K} r{r}: {weak} of {dlog.size} signs are weak"
        assert fragile <= SG.FRAGILE_CAP, f"{K} r{r}: {fragile} masks are fragile"
        strong = dlog >= SG.WEAK_DLOG
        assert np.array_equal(sign[strong], np.sign(SG.dlog64(y_hat, y, p)[r])[strong]), f"{K} r{r}: a strong sign differs"
        out[f"{K}_weak{r}"], out[f"{K}_fragile{r}"] = np.int64(weak), np.int64(fragile)
        out[f"{K}_signdiff{r}"] = np.int64((sign != np.sign(SG.dlog64(y_hat, y, p)[r])).sum())
        out[f"{K}_maskdiff{r}"] = np.int64((mask != (power >= SG.EPS)).sum())
        line.append(f"r{r} sc {float(out[f'{K}_relerr32_sc{r}']):.3g} mag {float(out[f'{K}_relerr32_mag{r}']):.3g} "
                    f"vjp {float(out[f'{K}_relerr32_vjp{r}']):.3g} weak {weak}/{dlog.size} fragile {fragile} "
                    f"below eps {int((power < SG.EPS).sum())} signdiff {int(out[f'{K}_signdiff{r}'])} "
                    f"maskdiff {int(out[f'{K}_maskdiff{r}'])}")
    if SG.stored(shape):
        for term, name in ((0, "sc"), (1, "mag")):
            a = _leaf(y_hat)
            loss(a, yt)[term].backward()
            out[f"{K}_grad_{name}"] = a.grad.numpy().astype(np.float32)
    print(f"{K}: " + "; ".join(line), flush=True)


def shape_case(waveform_loss, name, shape, out):
    S = SG.shape_key(name, shape)
    y_hat, y, winlens = SG.shape_case(name, shape)
    ties = [SG.shape_ties(y_hat, y, w) for w in winlens]
    if name in SG.BUILT:
        assert any(t[0 if name == "tie" else 1] > 0 for t in ties), f"{S}: the constructed case lost its point"
    else:
        assert all(t == (0, 0) for t in ties), f"{S}: tied or equal maxima {ties}"
    T = y.shape[-1]
    a = torch.from_numpy(y_hat.reshape(-1, 1, T)).clone().requires_grad_(True)
    waveform_loss.MultiWindowShapeLoss(winlens)(a, torch.from_numpy(y.reshape(-1, 1, T))).backward()
    g = a.grad.reshape(-1, T).numpy()
    exact = SG.shape_grad64(y_hat, y, winlens)
    assert np.array_equal(g != 0, exact != 0), f"{S}: the reference's nonzero pattern is not the first-index rule's"
    # float32 autograd: a few roundings of the largest term at a sample (terms of opposite sign may meet there and cancel)
    assert (np.abs(g - exact) <= 4 * 2.0 ** -24 * SG.shape_grad64(y_hat, y, winlens, magnitude=True)).all(), S
    if name in SG.BUILT or SG.stored(shape):
        out[f"{S}_grad"] = g.astype(np.float32)
    print(f"{S}: winlens {winlens} nonzero {int((g != 0).sum())} ties {ties}", flush=True)


def main():
    import_mel_loss()                                   # puts the reference on sys.path, with librosa or its stand-in
    from losses import stft_loss, waveform_loss
    torch.set_num_threads(4)
    out = {}
    for pname, shape in SG.CASES:
        stft_case(stft_loss, pname, shape, out)
    for wname, shape in SG.SHAPE_CASES:
        shape_case(waveform_loss, wname, shape, out)
    for name in SG.BUILT:
        shape_case(waveform_loss, name, None, out)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{OUT}: {os.path.getsize(OUT)} B")


if __name__ == "__main__":
    main()
