"""An exact model of the split-f16 conv arithmetic (audiodec_amd/csrc/conv_split16.h), and operands for which it has one right answer.

The kernels carry every f32 operand as v = hi + lo / 2048 (hi = f16(v), lo = f16((v - hi) * 2048)) and form

    model = sum hi_a hi_w + (sum hi_a lo_w + lo_a hi_w) / 2048 + bias + residual          (the lo_a lo_w / 2^22 term is dropped)

with f32 accumulators.  grid() draws operands n + m * 2^-14 (n a small integer, m in [-3, 3]): hi = n and lo = m / 8 are exact and lo is NOT
zero, every hi*hi product is an integer, every cross product a multiple of 2^-3, so cross / 2048 is a multiple of q = 2^-14.  LeakyReLU with a
power-of-two slope halves or quarters q.  Where

    S = sum |a(x)| |w| + |bias| + |residual|  <  2^23 q

every partial sum of the model -- in any order, in any grouping into accumulators, and the join fma(cross, 1/2048, main), the bias add and the
residual add after it -- is a multiple of q below 2^23 q, hence exactly representable in f32: the kernel's result does not depend on its
summation order and must be bit-equal to `model`.  model_conv / model_convtr compute the model in f64 (where all of the above is exact with
room to spare) and ASSERT the preconditions: operands equal to their split, S under the cap, the model representable in f32.

This is a plain helper module for tests/test_split16_model.py (CPU: the comparison is sharp) and tests/test_gpu_split16_exact.py."""
import torch
import torch.nn.functional as F

UNIT = 2.0 ** -14


def grid(rng, shape, nmax, density=1.0, mmax=3, unit=UNIT, signed=True):
    """float32 tensor of `shape`: a share `density` of the entries is n + m * unit with n an integer, 1 <= |n| <= nmax, and m an integer in
    [-mmax, mmax]; the rest is exactly 0.  signed=False: n > 0 only (an ELU in front is then the identity).  mmax = 0: the integer-only grid."""
    n = torch.randint(1, nmax + 1, shape, generator=rng).double()
    if signed:
        n = n * (torch.randint(0, 2, shape, generator=rng).double() * 2 - 1)
    m = torch.randint(-mmax, mmax + 1, shape, generator=rng).double()
    v = n + m * unit
    if density < 1.0:
        v = v * (torch.rand(shape, generator=rng) < density)
    return v.float()


def split(v):
    """(hi, lo) of the format, as program.pack_split16 forms them: f32 in, torch.half out (round to nearest even)."""
    v = v.float()
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    return hi, lo


def split_exact(v):
    """True where v == hi + lo / 2048 exactly."""
    hi, lo = split(v)
    return hi.double() + lo.double() / 2048.0 == v.double()


def act64(v, act, slope):
    v = v.double()
    if act is None:
        return v
    if act == "LeakyReLU":
        return torch.where(v > 0, v, v * slope)
    if act == "ELU":
        return F.elu(v)
    raise ValueError(act)


def grid_unit(act, slope, unit=UNIT):
    """q of the case: the grid unit of the activated operand times that of cross / 2048."""
    return unit * (slope if act == "LeakyReLU" else 1.0)


def parts(x_hist, w, act, slope, rep_groups=0):
    """The f64 tensors the model is built from: activated input a, its (hi, lo), the weights w, their (hi, lo).  rep_groups = g: the x.repeat
    form -- x_hist holds ONE group's channels, which every one of the g groups reads."""
    a = act64(x_hist, act, slope)
    if rep_groups:
        a = a.repeat(1, rep_groups, 1)
    ah, al = split(a)
    wh, wl = split(w)
    return a, ah.double(), al.double(), w.double(), wh.double(), wl.double()


def evaluate(conv, a, ah, al, w, wh, wl, bias, res):
    """(model, true conv, S) in f64, every output's: `conv(input, weight)` is the bias-free linear map.  No preconditions."""
    b = 0.0 if bias is None else bias.double().view(1, -1, 1)
    r = 0.0 if res is None else res.double()
    model = conv(ah, wh) + (conv(ah, wl) + conv(al, wh)) / 2048.0 + b + r
    true = conv(a, w) + b + r
    S = conv(a.abs(), w.abs()) + (0.0 if bias is None else bias.double().abs().view(1, -1, 1)) + (0.0 if res is None else res.double().abs())
    return model, true, S


def combine(conv, a, ah, al, w, wh, wl, bias, res, q):
    """(model as f32, true conv in f64, max S) after asserting the preconditions of the exactness argument."""
    model, true, S = evaluate(conv, a, ah, al, w, wh, wl, bias, res)
    assert bool((ah + al / 2048.0 == a).all()) and bool((wh + wl / 2048.0 == w).all()), "an operand is not equal to its split"
    assert float(S.max()) < 2.0 ** 23 * q, f"S = {float(S.max())} is not below the cap {2.0 ** 23 * q}"
    assert bool((model.float().double() == model).all()), "the model is not representable in f32"
    assert bool(((model / q).round() * q == model).all()), "the model is off the grid"
    return model.float(), true, float(S.max())


def _conv_map(stride, dilation, groups):
    return lambda p, q_: F.conv1d(p, q_, None, stride, 0, dilation, groups)


def _convtr_map(stride):
    return lambda p, q_: F.conv_transpose1d(p, q_, None, stride)[:, :, stride:-stride]


def model_conv(x_hist, w, bias, res, k, stride, dilation, groups, act, slope, rep=False, unit=UNIT):
    """CausalConv1d.inference on the window x_hist (B, cin, (k - 1) * dilation + L), the history in front: (model_f32, true_f64, max S).
    rep: x_hist holds cin_g channels and every group reads them (MultiGroupConv1d's x.repeat(1, groups, 1))."""
    assert w.shape[-1] == k
    return combine(_conv_map(stride, dilation, groups), *parts(x_hist, w, act, slope, groups if rep else 0), bias, res, grid_unit(act, slope, unit))


def model_convtr(x_hist, w, bias, stride, act, slope, unit=UNIT):
    """CausalConvTranspose1d.inference, kernel = 2 * stride, on the window x_hist (B, cin, 1 + L); w (cin, cout, 2 * stride)."""
    assert w.shape[-1] == 2 * stride
    return combine(_convtr_map(stride), *parts(x_hist, w, act, slope), bias, None, grid_unit(act, slope, unit))


def unchecked_conv(x_hist, w, bias, res, k, stride, dilation, groups, act, slope):
    """model_conv for operands off the grid (the format's edges): (model, true, S) per output in f64, nothing asserted."""
    return evaluate(_conv_map(stride, dilation, groups), *parts(x_hist, w, act, slope), bias, res)


def unchecked_convtr(x_hist, w, bias, stride, act, slope):
    return evaluate(_convtr_map(stride), *parts(x_hist, w, act, slope), bias, None)


def rounding_set(rng, shape):
    """Activations whose lo half does NOT fit f16, so that the split has to round it.  An f32 has 24 significant bits, hi takes 11, the
    remainder has a sign and up to 12: one more than lo holds, and only where 0.5 <= |(v - hi) * 2048| < 1 -- every inexact lo is a TIE.
    All of these are such ties: v = +-(1 + i 2^-10 +- (1/2 + t 2^-11 + 2^-12) / 2048), three quarters of them with t odd (to nearest even
    is away from zero: a truncating split is off by one lo ulp), the rest with t even (a split rounding ties away is off).  v is not equal to
    its split; what a kernel that multiplies by exact +-1 weights (lo = 0, one non-zero per row) must return is joined(v)."""
    i = torch.randint(0, 1024, shape, generator=rng).double()
    t = torch.randint(0, 255, shape, generator=rng).double() * 2 + (torch.rand(shape, generator=rng) < 0.75).double()
    s1 = torch.randint(0, 2, shape, generator=rng).double() * 2 - 1
    s2 = torch.randint(0, 2, shape, generator=rng).double() * 2 - 1
    v = s1 * (1.0 + i * 2.0 ** -10 + s2 * (0.5 + t * 2.0 ** -11 + 2.0 ** -12) / 2048.0)
    assert bool((v.float().double() == v).all())
    return v.float()


def joined(v):
    """hi + lo / 2048 of v as f32 (exact: at most 23 significant bits where |lo| < 1 <= |hi| ... checked)."""
    hi, lo = split(v)
    y = hi.double() + lo.double() / 2048.0
    assert bool((y.float().double() == y).all())
    return y.float()
