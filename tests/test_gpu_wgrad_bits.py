"""GPU: the three weight-gradient GEMMs (enc_grad.hip's wgrad_kernel, dec_wgrad.hip's convtr_wgrad_kernel, disc_wgrad.hip's
disc_wgrad_kernel) bit for bit against a recorded commit, on full-mantissa operands.

The exact tests of the three kernels use small integers, whose sums are exact in any order; this file sees a change of the
summation order.  tests/golden/wgrad_bits.json holds, per case, the sha256 of the raw bytes of dW and of db that the commit
PARENT computed (tests/golden/make_wgrad_bits.py wrote it from that commit's build); the kernels must still compute those bytes.
The digests are a record of that commit, never of the code under test: the file is not regenerated when a kernel changes.

Operands come from `_values`: a closed-form integer hash of the element index (no library random stream), made into f32
values with all 23 mantissa bits, either sign and magnitudes from 2^-3 to 2^2; the discriminator's saved output y also has
exact zeros.  Every case is also held against an f64 torch restatement of the same sums, within
    (n_terms + 4) 2^-23 sum|terms|
per element: n_terms products accumulated in f32 in some order lose at most one rounding of the running sum, itself at most
sum|terms|, per addition; the + 4 covers the rounding of an operand's activation (expm1_neg: 1.2 ulp, LeakyReLU's product and
the mask's: 1/2 ulp each) and the one rounding of the f64 fold.  An analytic bound, loose on purpose: it only shows that the
recorded digest is not one of garbage.

Cases (CONV, CONVTR, DISC): per kernel, M per group of 5, 65 and 130 (the three tile shapes, each with a partial last row
tile); ck of 127 and 128 (db's column on either side of the 128-column tile edge; without db a whole column tile goes), ck < 32
and ck of 129 / 130; db asked for and not; groups 1 and 2; S = 3 slices with a short last slice (13 steps: 5, 5, 3) and S = 1,
reduction lengths that are no multiple of 32 with item boundaries inside a step; n_items = 0 (dW and db exactly zero).
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PARENT = "29fc7f407a68242b82aa731283cc27db060d99d8"       # the commit whose build wrote wgrad_bits.json
NONE, ELU, LEAKY = 0, 1, 2
ALPHA = {NONE: 0.0, ELU: 0.75, LEAKY: 0.1}

# ---- the cases ----
# causal conv: (entry, groups, c_in/g, c_out/g, kernel, dilation, stride, T, n_items, act, db asked for, slices)
# adk_conv_wgrad: one group, none / ELU, any stride; adk_voc_conv_wgrad: groups, none / ELU / LeakyReLU, stride 1
CONV = {
    "ck127_m5_S3":         ("adk_conv_wgrad", 1, 127, 5, 1, 1, 1, 131, 3, NONE, True, 3),
    "ck128_m65_S3":        ("adk_conv_wgrad", 1, 128, 65, 1, 1, 1, 131, 3, ELU, True, 3),
    "ck128_m65_S3_nodb":   ("adk_conv_wgrad", 1, 128, 65, 1, 1, 1, 131, 3, ELU, False, 3),
    "ck127_m130_nodb":     ("adk_conv_wgrad", 1, 127, 130, 1, 1, 1, 45, 2, ELU, False, 1),
    "k7s2_m130_S3":        ("adk_conv_wgrad", 1, 3, 130, 7, 1, 2, 261, 3, ELU, True, 3),
    "k3d9_short_m5":       ("adk_conv_wgrad", 1, 4, 5, 3, 9, 1, 13, 7, NONE, True, 1),        # T 13 < 19: tap 0 is never live
    "k7d9_short_m65_S3":   ("adk_conv_wgrad", 1, 3, 65, 7, 9, 1, 20, 20, ELU, True, 3),       # T 20 < 55: taps 0..4 never live
    "k3s2_ck129_m5":       ("adk_conv_wgrad", 1, 43, 5, 3, 1, 2, 90, 2, NONE, True, 1),
    "k7d9s2_m130_nodb":    ("adk_conv_wgrad", 1, 5, 130, 7, 9, 2, 30, 5, ELU, False, 1),
    "voc_g2_ck127_m5_S3":  ("adk_voc_conv_wgrad", 2, 127, 5, 1, 1, 1, 131, 3, LEAKY, True, 3),
    "voc_g2_ck128_m65_nodb": ("adk_voc_conv_wgrad", 2, 128, 65, 1, 1, 1, 45, 2, LEAKY, False, 1),
    "voc_g2_ck128_m130_S3": ("adk_voc_conv_wgrad", 2, 128, 130, 1, 1, 1, 131, 3, ELU, True, 3),
    "voc_g2_k7d9_m65_S3":  ("adk_voc_conv_wgrad", 2, 3, 65, 7, 9, 1, 20, 20, LEAKY, True, 3),
    "voc_g2_k3_m130_nodb": ("adk_voc_conv_wgrad", 2, 4, 130, 3, 1, 1, 45, 2, NONE, False, 1),
    "voc_g1_k7_ck63_m5_S3": ("adk_voc_conv_wgrad", 1, 9, 5, 7, 1, 1, 131, 3, LEAKY, True, 3),
    "voc_g2_k3d9_ck129_m5_S3": ("adk_voc_conv_wgrad", 2, 43, 5, 3, 9, 1, 131, 3, ELU, True, 3),
    "no_items":            ("adk_conv_wgrad", 1, 4, 5, 3, 1, 2, 13, 0, ELU, True, 1),
    "voc_no_items":        ("adk_voc_conv_wgrad", 2, 4, 65, 3, 1, 1, 13, 0, LEAKY, False, 1),
}
# transposed conv, kernel = 2 stride: (entry, c_in, c_out, stride, T, n_items, act, db asked for, slices)
# c_out 23 at stride 3 (138 columns, 6 per channel): the second tile's first column is inside a channel; 17 at stride 8: three tiles
CONVTR = {
    "s3_T1_m5":            ("adk_convtr_wgrad", 5, 23, 3, 1, 45, NONE, True, 1),
    "s3_T2_m65_S3":        ("adk_convtr_wgrad", 65, 23, 3, 2, 200, ELU, True, 3),
    "s8_m130_S3_nodb":     ("adk_convtr_wgrad", 130, 9, 8, 131, 3, ELU, False, 3),
    "s2_T2_m5":            ("adk_convtr_wgrad", 5, 33, 2, 2, 45, ELU, True, 1),
    "s2_m65_S3_nodb":      ("adk_convtr_wgrad", 65, 33, 2, 131, 3, NONE, False, 3),
    "voc_s3_T1_m65_S3":    ("adk_voc_convtr_wgrad", 65, 5, 3, 1, 400, LEAKY, True, 3),
    "voc_s2_T2_m130_nodb": ("adk_voc_convtr_wgrad", 130, 33, 2, 2, 45, LEAKY, False, 1),
    "voc_s8_T2_m5_S3":     ("adk_voc_convtr_wgrad", 5, 9, 8, 2, 200, NONE, True, 3),
    "voc_s3_m130_S3":      ("adk_voc_convtr_wgrad", 130, 23, 3, 131, 3, LEAKY, True, 3),
    "voc_s8_T1_m65":       ("adk_voc_convtr_wgrad", 65, 17, 8, 1, 45, ELU, True, 1),
    "no_items":            ("adk_convtr_wgrad", 5, 23, 3, 2, 0, ELU, True, 1),
    "voc_no_items":        ("adk_voc_convtr_wgrad", 65, 9, 8, 1, 0, LEAKY, False, 1),
}
# discriminator: (groups, c_in/g, c_out/g, kernel, stride, pad, period, h_in, n_items, act, db asked for, slices)
# (5, 3, 2) and (5, 3, 0) always with h_in + 2 pad - k no multiple of 3: rows of x the forward never reached
DISC = {
    "k5s3p2_P3_m5_S3":     (1, 3, 5, 5, 3, 2, 3, 128, 3, LEAKY, True, 3),
    "g2_k3_ck129_P2_m65_S3": (2, 43, 65, 3, 1, 1, 2, 65, 3, LEAKY, True, 3),
    "k5s3p0_ck130_m130_S3_nodb": (1, 26, 130, 5, 3, 0, 1, 396, 3, NONE, False, 3),
    "g2_k5s3p2_hin2_ck125_m5": (2, 25, 5, 5, 3, 2, 1, 2, 45, LEAKY, True, 1),                # h_in 2 < k 5: legal by the padding
    "k1_ck127_P3_m65":     (1, 127, 65, 1, 1, 0, 3, 15, 2, LEAKY, True, 1),
    "k1_ck128_P2_m130":    (1, 128, 130, 1, 1, 0, 2, 22, 2, NONE, True, 1),
    "k1_ck128_P2_m130_nodb": (1, 128, 130, 1, 1, 0, 2, 22, 2, LEAKY, False, 1),
    "g2_k3_hin1_P3_m130_nodb": (2, 4, 130, 3, 1, 1, 3, 1, 30, LEAKY, False, 1),              # h_in 1 < k 3
    "k5s3p0_P2_m65":       (1, 5, 65, 5, 3, 0, 2, 12, 15, NONE, True, 1),
    "g2_k5s3p2_P1_m65":    (2, 3, 65, 5, 3, 2, 1, 128, 3, LEAKY, True, 1),
    "k3_P1_m5_S3_nodb":    (1, 4, 5, 3, 1, 1, 1, 131, 3, NONE, False, 3),
    "g2_k5s3p0_P3_m130_S3": (2, 2, 130, 5, 3, 0, 3, 132, 3, LEAKY, True, 3),
    "no_items":            (2, 3, 5, 5, 3, 2, 3, 20, 0, LEAKY, True, 1),
}
ALL = [("conv", k) for k in CONV] + [("convtr", k) for k in CONVTR] + [("disc", k) for k in DISC]


# ---- operands ----
def _values(salt, shape, zeros=False):
    """f32 tensor of `shape`: element i is made of the 32-bit hash h(i) = mix((i + 1) * 0x9E3779B1 + salt * 0x85EBCA6B)
    (mix: the xor-shift-multiply finaliser below, all mod 2^32): sign from bit 31, exponent 2^-3 .. 2^2 from bits 23..30 mod 6, the 23
    mantissa bits from bits 0..22.  zeros: every element whose hash is 0 mod 7 becomes an exact 0."""
    n = int(np.prod(shape))
    m = np.uint64(0xFFFFFFFF)
    h = ((np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B1)) + np.uint64((salt * 0x85EBCA6B) & 0xFFFFFFFF)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & m
    h ^= h >> np.uint64(16)
    mant = (h & np.uint64(0x7FFFFF)).astype(np.float64) / float(1 << 23)
    expo = (((h >> np.uint64(23)) & np.uint64(0xFF)) % np.uint64(6)).astype(np.int64) - 3
    sign = np.where((h >> np.uint64(31)) & np.uint64(1), -1.0, 1.0)
    v = sign * (1.0 + mant) * np.exp2(expo.astype(np.float64))              # 24 significant bits: exact in f32
    if zeros:
        v[h % np.uint64(7) == 0] = 0.0
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return torch.from_numpy(out.reshape(shape))


def _salt(kind, name):
    return int.from_bytes(hashlib.sha256(f"{kind}/{name}".encode()).digest()[:4], "little")


def _act64(x, act, alpha):
    """The input activation in f64, alpha the f32 value the kernel is given."""
    a = float(np.float32(alpha))
    if act == ELU:
        return torch.where(x > 0, x, a * torch.expm1(x))
    if act == LEAKY:
        return torch.where(x > 0, x, a * x)
    return x


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nan(gpu, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _dev(gpu, t):
    return t.to(gpu).contiguous() if t.numel() else None


# ---- one case on the HIP path, and its f64 restatement ----
# Each _run_* gives (dw, db or None, plan's slices, (dW64, sum|terms| of dW, n_terms), (db64, sum|terms| of db, n_terms)).
def _grad_of(conv, a, g, wshape):
    """d/dw of <conv(a, w), g> at w = 0 in f64: the weight gradient's sums, whatever they are made of."""
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    if a.shape[0] == 0:
        return torch.zeros(wshape, dtype=torch.float64)
    conv(a, w).backward(g)
    return w.grad


def _conv_ref(x, dy, G, k, d, s, act, alpha):
    def conv(a, w):
        return F.conv1d(F.pad(a, ((k - 1) * d, 0)), w, None, stride=s, dilation=d, groups=G)
    a64, g64, shape, terms = _act64(x.double(), act, alpha), dy.double(), (dy.shape[1], x.shape[1] // G, k), dy.shape[0] * dy.shape[2]
    return (_grad_of(conv, a64, g64, shape), _grad_of(conv, a64.abs(), g64.abs(), shape), terms), \
        (g64.sum((0, 2)), g64.abs().sum((0, 2)), terms)


def _convtr_ref(x, dy, s, act, alpha):
    t = x.shape[2]

    def conv(a, w):                                        # frame 0 replicated to the left, the first s samples cropped
        return F.conv_transpose1d(torch.cat([a[:, :, :1], a], 2), w, None, stride=s)[:, :, s:s + t * s]
    a64, g64, shape = _act64(x.double(), act, alpha), dy.double(), (x.shape[1], dy.shape[1], 2 * s)
    return (_grad_of(conv, a64, g64, shape), _grad_of(conv, a64.abs(), g64.abs(), shape), 2 * x.shape[0] * t), \
        (g64.sum((0, 2)), g64.abs().sum((0, 2)), 1)        # db is an f64 sum rounded once


def _disc_ref(x, dy, y, G, k, s, pad, act, slope):
    def conv(a, w):
        return F.conv2d(a, w[..., None], None, stride=(s, 1), padding=(pad, 0), groups=G)
    dz = dy.double() * (torch.where(y > 0, 1.0, float(np.float32(slope))).double() if act == LEAKY else 1.0)
    x64, shape, terms = x.double(), (dy.shape[1], x.shape[1] // G, k), dy.shape[0] * dy.shape[2] * dy.shape[3]
    return (_grad_of(conv, x64, dz, shape), _grad_of(conv, x64.abs(), dz.abs(), shape), terms), \
        (dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), terms)


def _run_conv(gpu, name):
    from audiodec_amd import native
    entry, G, cig, cog, k, d, s, t, n, act, want_db, _ = CONV[name]
    c_in, c_out, t_out, alpha = G * cig, G * cog, (t - 1) // s + 1, ALPHA[act]
    salt = _salt("conv", name)
    x, dy = _values(salt, (n, c_in, t)), _values(salt + 1, (n, c_out, t_out))
    lib, ws_b, sl = native.lib(), C.c_int64(0), C.c_int32(0)
    last = s if entry == "adk_conv_wgrad" else G             # the plan's and the call's one differing argument
    native.check(getattr(lib, entry + "_plan")(n, c_in, t, c_out, k, d, last, C.byref(ws_b), C.byref(sl)), entry + "_plan")
    ws, dw, db = _nan(gpu, max(1, ws_b.value // 4)), _nan(gpu, c_out, cig, k), (_nan(gpu, c_out) if want_db else None)
    dyg, xg = _dev(gpu, dy), _dev(gpu, x)
    native.check(getattr(lib, entry)(_p(dyg), _p(xg), _p(dw), _p(db), _p(ws), n, c_in, t, c_out, k, d, last, act, C.c_float(alpha),
                                     native.current_stream(gpu)), entry)
    return (dw, db, sl.value) + _conv_ref(x, dy, G, k, d, s, act, alpha)


def _run_convtr(gpu, name):
    from audiodec_amd import native
    entry, c_in, c_out, s, t, n, act, want_db, _ = CONVTR[name]
    alpha, salt = ALPHA[act], _salt("convtr", name)
    x, dy = _values(salt, (n, c_in, t)), _values(salt + 1, (n, c_out, t * s))
    lib, ws_b, sl = native.lib(), C.c_int64(0), C.c_int32(0)
    native.check(lib.adk_convtr_wgrad_plan(n, c_in, t, c_out, 2 * s, s, C.byref(ws_b), C.byref(sl)), "adk_convtr_wgrad_plan")
    ws, dw, db = _nan(gpu, max(2, ws_b.value // 4)), _nan(gpu, c_in, c_out, 2 * s), (_nan(gpu, c_out) if want_db else None)
    dyg, xg = _dev(gpu, dy), _dev(gpu, x)
    native.check(getattr(lib, entry)(_p(dyg), _p(xg), _p(dw), _p(db), _p(ws), n, c_in, t, c_out, 2 * s, s, act, C.c_float(alpha),
                                     native.current_stream(gpu)), entry)
    return (dw, db, sl.value) + _convtr_ref(x, dy, s, act, alpha)


def _run_disc(gpu, name):
    from audiodec_amd import native
    G, cig, cog, k, s, pad, period, h_in, n, act, want_db, _ = DISC[name]
    c_in, c_out, h_out, slope = G * cig, G * cog, (h_in + 2 * pad - k) // s + 1, ALPHA[act]
    salt = _salt("disc", name)
    x, dy, y = _values(salt, (n, c_in, h_in, period)), _values(salt + 1, (n, c_out, h_out, period)), \
        _values(salt + 2, (n, c_out, h_out, period), zeros=True)
    if n:
        assert bool((y == 0).any()) and bool((y > 0).any()) and bool((y < 0).any())
    lib, ws_b, sl = native.lib(), C.c_int64(0), C.c_int32(0)
    native.check(lib.adk_disc_conv_wgrad_plan(n, c_in, h_in, period, c_out, G, k, s, pad, C.byref(ws_b), C.byref(sl)),
                 "adk_disc_conv_wgrad_plan")
    ws, dw, db = _nan(gpu, max(1, ws_b.value // 4)), _nan(gpu, c_out, cig, k), (_nan(gpu, c_out) if want_db else None)
    dyg, yg, xg = _dev(gpu, dy), (_dev(gpu, y) if act == LEAKY else None), _dev(gpu, x)
    native.check(lib.adk_disc_conv_wgrad(_p(dyg), _p(yg), _p(xg), _p(dw), _p(db), _p(ws), n, c_in, h_in, period, c_out, G, k, s, pad, act,
                                         C.c_float(slope), native.current_stream(gpu)), "adk_disc_conv_wgrad")
    return (dw, db, sl.value) + _disc_ref(x, dy, y, G, k, s, pad, act, slope)


RUN = {"conv": _run_conv, "convtr": _run_convtr, "disc": _run_disc}
TABLE = {"conv": CONV, "convtr": CONVTR, "disc": DISC}


def digest(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(gpu, kind, name):
    """Runs one case, checks the plan's slices and the f64 restatement, and gives (dw, db) on the device."""
    dw, db, slices, ref_w, ref_b = RUN[kind](gpu, name)
    assert slices == TABLE[kind][name][-1], f"{kind}/{name}: the plan gives {slices} slices"
    for what, got, (want, mag, terms) in (("dW", dw, ref_w), ("db", db, ref_b)):
        if got is None:
            continue
        err = (got.cpu().double() - want).abs()
        bound = (terms + 4) * 2.0 ** -23 * mag
        worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() and float(mag.max()) > 0 else 0.0
        print(f"{kind}/{name} {what}: max|hip - f64| {float(err.max()):.3g}  largest fraction of the bound {worst:.3f}")
        assert bool((err <= bound).all()), f"{kind}/{name} {what}: {float(err.max()):.3g} outside (n + 4) 2^-23 sum|terms|"
    return dw, db


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "wgrad_bits.json")) as fh:
        rec = json.load(fh)
    assert rec.get("parent_commit") == PARENT, "wgrad_bits.json must be the record of the commit this file names"
    assert sorted(rec["cases"]) == sorted(f"{kind}/{name}" for kind, name in ALL)
    return rec["cases"]


def test_cases_cover_the_list():
    for kind, table, m_at, db_at in (("conv", CONV, 3, 10), ("convtr", CONVTR, 1, 7), ("disc", DISC, 2, 10)):
        live = [v for v in table.values() if v[{"conv": 8, "convtr": 5, "disc": 8}[kind]] > 0]
        assert {v[m_at] for v in live} == {5, 65, 130}, kind
        assert {v[db_at] for v in live} == {True, False} and {v[-1] for v in live} == {1, 3}, kind
        for m in (5, 65, 130):                             # every tile shape with several slices and with one
            assert {v[-1] for v in live if v[m_at] == m} == {1, 3}, (kind, m)
    conv = list(CONV.values())
    assert {v[2] * v[4] for v in conv} >= {127, 128, 129} and min(v[2] * v[4] for v in conv) < 32
    assert {v[4] for v in conv} == {1, 3, 7} and {v[5] for v in conv} == {1, 9} and {v[6] for v in conv} == {1, 2}
    assert {v[1] for v in conv} == {1, 2} and {(v[0], v[9]) for v in conv} == {
        ("adk_conv_wgrad", NONE), ("adk_conv_wgrad", ELU), ("adk_voc_conv_wgrad", NONE), ("adk_voc_conv_wgrad", ELU),
        ("adk_voc_conv_wgrad", LEAKY)}
    assert any(v[7] <= (v[4] - 1) * v[5] for v in conv)    # T shorter than the receptive field
    tr = list(CONVTR.values())
    assert {v[3] for v in tr} == {2, 3, 8} and {1, 2} <= {v[4] for v in tr}
    assert any(128 % (2 * v[3]) and v[2] * 2 * v[3] > 128 for v in tr)
    assert {(v[0], v[6]) for v in tr} == {("adk_convtr_wgrad", NONE), ("adk_convtr_wgrad", ELU), ("adk_voc_convtr_wgrad", NONE),
                                          ("adk_voc_convtr_wgrad", ELU), ("adk_voc_convtr_wgrad", LEAKY)}
    di = list(DISC.values())
    assert {v[6] for v in di} == {1, 2, 3} and {v[3:6] for v in di} >= {(5, 3, 2), (3, 1, 1), (5, 3, 0)}
    assert all((v[7] + 2 * v[5] - v[3]) % v[4] for v in di if v[4] == 3) and any(v[7] < v[3] for v in di)
    assert {v[1] * v[3] for v in di} >= {127, 128, 129, 130} and {v[0] for v in di} == {1, 2} and {v[9] for v in di} == {NONE, LEAKY}
    assert 40 <= len(ALL) <= 60


@pytest.mark.parametrize("kind,name", ALL, ids=[f"{k}-{n}" for k, n in ALL])
def test_bits_are_the_recorded_commits(gpu, recorded, kind, name):
    dw, db = run_case(gpu, kind, name)
    want = recorded[f"{kind}/{name}"]
    if "no_items" in name:                                 # no live step: compared directly, not by digest
        assert not dw.any() and (db is None or not db.any())
    assert digest(dw) == want["dw"], f"{kind}/{name}: dW is not bitwise the recorded commit's"
    assert digest(db) == want["db"], f"{kind}/{name}: db is not bitwise the recorded commit's"
