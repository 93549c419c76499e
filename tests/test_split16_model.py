"""The exact model of the split-f16 convs (tests/split16_model.py) is sharp: proved on the CPU, so that nobody needs a GPU to trust the
bit-for-bit comparison of tests/test_gpu_split16_exact.py.

* An emulation of what the kernels do -- 16-k chunks accumulated in f32, in a shuffled order, into acc0 (hi*hi) and acc1 (the cross
  products), then fma(acc1, 1/2048, acc0), bias, residual, all in f32 -- equals the model bit for bit.
* The wrong kernels one can think of (MUTANTS) each differ from the model on at least half of the outputs of at least one case.
* The integer-only grid (m = 0, every lo half zero) does NOT see the cross term deleted: the reason the grid has a second level.

`lo` truncated toward zero instead of rounded cannot be shown on the two-level grid, nor on a finer one (|m| <= 7 on a 2^-15 grid): there
lo is exactly representable in f16 and no rounding takes place at all (asserted below).  That mutant is shown on
split16_model.rounding_set: activations with a 13-bit lo, multiplied by a signed permutation (weights +-1, lo = 0), for which the right
answer is still exact -- hi + lo / 2048 with lo rounded to nearest even."""
import pytest
import torch

import split16_model as M

# cin_g, cout_g, groups, k, stride, dilation, act, slope, x density, B, L (output steps), bias, residual
CASES = {
    "K96 dense-ish groups 3": (32, 32, 3, 3, 1, 1, None, 0.0, 0.4, 3, 20, True, True),
    "K448 dilation 9 slope 0.5": (64, 64, 1, 7, 1, 9, "LeakyReLU", 0.5, 0.05, 2, 24, True, False),
    "K896 slope 0.25": (128, 32, 1, 7, 1, 1, "LeakyReLU", 0.25, 0.015, 2, 16, False, True),
    "K320 stride 5": (32, 64, 1, 10, 5, 1, None, 0.0, 0.15, 2, 8, True, False),
    "K2816": (256, 32, 1, 11, 1, 1, None, 0.0, 0.018, 2, 12, True, True),
    "K2816 slope 0.5": (256, 32, 1, 11, 1, 1, "LeakyReLU", 0.5, 0.009, 2, 12, True, False),
    "K704 ELU on x >= 0, groups 2": (64, 32, 2, 11, 1, 1, "ELU", 0.0, 0.04, 2, 12, False, False),
}


def tensors(name, mmax=3, unit=M.UNIT):
    cin_g, cout_g, groups, k, stride, dil, act, slope, density, B, L, has_bias, has_res = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = M.grid(g, (B, cin_g * groups, (k - 1) * dil + L * stride), 4, density, mmax, unit, signed=act != "ELU")
    w = M.grid(g, (cout_g * groups, cin_g, k), 3, 1.0, mmax, unit)
    bias = M.grid(g, (cout_g * groups,), 4, 1.0, mmax, unit) if has_bias else None
    res = M.grid(g, (B, cout_g * groups, L), 4, 1.0, mmax, unit) if has_res else None
    return x, w, bias, res


def model_of(name, x, w, bias, res, unit=M.UNIT):
    cin_g, cout_g, groups, k, stride, dil, act, slope = CASES[name][:8]
    return M.model_conv(x, w, bias, res, k, stride, dil, groups, act, slope, unit=unit)


@pytest.fixture(scope="module")
def models():
    """Every case's operands and model, computed once and left unchanged."""
    out = {}
    for name in CASES:
        t = tensors(name)
        out[name] = (t, model_of(name, *t))
    return out


def emulate(name, x, w, bias, res, seed):
    """The kernels' arithmetic in f32: chunks of 16 k in a shuffled order, two accumulators, the join, bias, residual."""
    cin_g, cout_g, groups, k, stride, dil, act, slope = CASES[name][:8]
    a = M.act64(x, act, slope).float()
    ah, al = (t.float() for t in M.split(a))
    wh, wl = (t.float() for t in M.split(w))
    B = x.shape[0]

    def cols(t):                                          # (B, cin, rows) -> (groups, N, cin_g * k)
        u = t.unfold(2, (k - 1) * dil + 1, stride)[..., ::dil]                      # (B, cin, L, k)
        return u.permute(1, 3, 0, 2).reshape(groups, cin_g * k, -1).transpose(1, 2).contiguous()

    def rows(t):                                          # (cout, cin_g, k) -> (groups, cout_g, cin_g * k)
        return t.reshape(groups, cout_g, cin_g * k)

    Ah, Al, Wh, Wl = cols(ah), cols(al), rows(wh), rows(wl)
    K = cin_g * k
    assert K % 16 == 0
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(K // 16, generator=g).tolist()
    n = Ah.shape[1]
    acc0 = torch.zeros(groups, n, cout_g)
    acc1 = torch.zeros(groups, n, cout_g)
    for c in order:
        s = slice(16 * c, 16 * c + 16)
        acc0 = acc0 + torch.bmm(Ah[:, :, s], Wh[:, :, s].transpose(1, 2))
        acc1 = acc1 + torch.bmm(Ah[:, :, s], Wl[:, :, s].transpose(1, 2))
        acc1 = acc1 + torch.bmm(Al[:, :, s], Wh[:, :, s].transpose(1, 2))
    y = acc1 * (1.0 / 2048.0) + acc0                      # acc1 / 2048 is exact (a power of two): one rounding, as the fma
    y = y.reshape(groups, B, -1, cout_g).permute(1, 0, 3, 2).reshape(B, groups * cout_g, -1)
    if bias is not None:
        y = y + bias.view(1, -1, 1)
    if res is not None:
        y = y + res
    return y


@pytest.mark.parametrize("name", list(CASES))
def test_shuffled_f32_accumulation_reproduces_the_model(models, name):
    (x, w, bias, res), (model, true, S) = models[name]
    assert model.dtype == torch.float32 and bool((model.double() - true).abs().max() < 1e-3)
    for seed in (1, 2):
        assert torch.equal(emulate(name, x, w, bias, res, seed), model), (name, seed)
    # the model is not the f32-rounded true conv: the dropped lo*lo term is visible, so the test tells this arithmetic from an exact-f32 one
    print(f"{name}: S = {S:.1f}, model != f32(true conv) on {float((model != true.float()).float().mean()):.1%} of the outputs")


def test_transposed_model_is_the_oracles_transposed_conv():
    """model_convtr's true conv against the oracle's CausalConvTranspose1d.inference, and its preconditions on a dense 64-channel case."""
    from oracle import audiodec_oracle as O
    g = torch.Generator().manual_seed(3)
    for cin, cout, s, density in ((64, 32, 3, 0.2), (128, 8, 5, 0.1)):
        x = M.grid(g, (2, cin, 1 + 6), 4, density)
        w = M.grid(g, (cin, cout, 2 * s), 3)
        bias = M.grid(g, (cout,), 4)
        model, true, S = M.model_convtr(x, w, bias, s, "LeakyReLU", 0.5)
        a = M.act64(x, "LeakyReLU", 0.5)
        ref, _ = O.causal_convtr1d_inference(a[:, :, 1:], a[:, :, :1], w.double(), bias.double(), s)
        assert torch.equal(true, ref) and model.shape == (2, cout, 6 * s)


# ---- the wrong kernels ----
def _mutant(name, x, w, bias, res, kind):
    cin_g, cout_g, groups, k, stride, dil, act, slope = CASES[name][:8]
    a, ah, al, w64, wh, wl = M.parts(x, w, act, slope)
    F = torch.nn.functional
    b = 0.0 if bias is None else bias.double().view(1, -1, 1)
    r = 0.0 if res is None else res.double()

    def conv(p, q, d=dil):
        return F.conv1d(p, q, None, stride, 0, d, groups)

    def full(ah_, al_, wh_, wl_, scale=2048.0, d=dil):
        return conv(ah_, wh_, d) + (conv(ah_, wl_, d) + conv(al_, wh_, d)) / scale + b + r

    if kind == "cross term dropped":
        y = conv(ah, wh) + b + r
    elif kind == "only hi_a*lo_w kept":
        y = conv(ah, wh) + conv(ah, wl) / 2048.0 + b + r
    elif kind == "lo scaled by 1/1024":
        y = full(ah, al, wh, wl, 1024.0)
    elif kind == "one tap shifted by one row":
        if k < 2:
            return None
        j = k // 2

        def shift(t):                                     # tap j reads the row before its own
            t = t.clone()
            t[..., j - 1] += t[..., j]
            t[..., j] = 0
            return t

        y = full(ah, al, shift(wh), shift(wl))
    elif kind in ("dilation + 1", "dilation - 1"):
        d = dil + (1 if kind.endswith("+ 1") else -1)
        if d < 1 or k < 2:
            return None
        grow = (k - 1) * (d - dil)                        # the causal window ends where it ended: rows are added or dropped in front

        def fit(t):
            return F.pad(t, (grow, 0)) if grow > 0 else t[:, :, -grow:]

        y = full(fit(ah), fit(al), wh, wl, d=d)
    elif kind == "a group reads its neighbour's channels":
        if groups < 2:
            return None
        y = full(ah.roll(cin_g, 1), al.roll(cin_g, 1), wh, wl)
    else:
        raise ValueError(kind)
    return y.float()


MUTANTS = ["cross term dropped", "only hi_a*lo_w kept", "lo scaled by 1/1024", "one tap shifted by one row", "dilation + 1", "dilation - 1",
           "a group reads its neighbour's channels"]


def test_every_mutant_is_rejected(models):
    """Share of outputs on which each wrong kernel differs from the model, per case; at least half somewhere."""
    table = {}
    for kind in MUTANTS:
        shares = {}
        for name, ((x, w, bias, res), (model, _, _)) in models.items():
            y = _mutant(name, x, w, bias, res, kind)
            if y is not None:
                shares[name] = float((y != model).float().mean())
        table[kind] = shares
        print(f"{kind:40s} best {max(shares.values()):6.1%}   " + "  ".join(f"{v:.0%}" for v in shares.values()))
    for kind, shares in table.items():
        assert shares and max(shares.values()) >= 0.5, (kind, shares)


def test_the_integer_grid_is_blind_to_the_cross_term():
    """With m = 0 every lo half is zero: a kernel without the cross term passes on every case.  Hence the second level."""
    for name in CASES:
        x, w, bias, res = tensors(name, mmax=0)
        model, _, _ = model_of(name, x, w, bias, res)
        assert not bool(M.split(x)[1].any()) and not bool(M.split(w)[1].any())
        assert torch.equal(_mutant(name, x, w, bias, res, "cross term dropped"), model), name


def _half_toward_zero(v):
    """f16(v) rounded toward zero."""
    h = v.float().half()
    over = h.float().abs() > v.float().abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.half)           # sign-magnitude: one step down in magnitude


def test_truncated_lo_shows_on_the_rounding_set_only():
    g = torch.Generator().manual_seed(9)
    # on the grids lo is exact in f16: rounding it toward zero changes nothing, so no grid case can tell
    for unit, mmax in ((M.UNIT, 3), (2.0 ** -15, 7)):
        v = M.grid(g, (4096,), 4, 1.0, mmax, unit)
        hi, lo = M.split(v)
        assert bool(M.split_exact(v).all()) and bool(lo.any())
        assert torch.equal(_half_toward_zero((v - hi.float()) * 2048.0), lo)
    # the rounding set: the split rounds lo, and the truncating kernel is off on more than half of the outputs
    v = M.rounding_set(g, (4096,))
    hi, lo = M.split(v)
    assert not bool(M.split_exact(v).any())
    want = M.joined(v)
    got = (hi.double() + _half_toward_zero((v - hi.float()) * 2048.0).double() / 2048.0).float()
    share = float((got != want).float().mean())
    print(f"{'lo truncated toward zero':40s} {share:6.1%} of the rounding set")
    assert share >= 0.5
    # and what the format promises for them: 2^-22 relative
    assert float(((want.double() - v.double()).abs() / v.double().abs()).max()) <= 2.0 ** -22
