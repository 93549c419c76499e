"""conv_rk16 (csrc/conv_rk16.hip): the whole-tile, rows-once-in-LDS split-f16 kernel that launch_conv_sk16 hands the wide-group convs
of several steps per stream -- against the same causal conv in fp64 on the CPU (CausalConv1d.inference, layers/conv_layer.py:153-156),
against the stream-K split-f16 launch on identical operands (option "conv_rk16" = 0), against itself, and with / without a shadow ring.

Option value 2 lifts the kernel's launch-size floor (by default it takes launches of >= 192 tiles only), "gv16_max_columns" = 0 keeps
the few-column kernel out of the way, so that the small shapes here reach it: stream counts at which a 64-column tile starts and ends
inside a stream (13 and 14 streams x 5 steps = 65 / 70 columns, 27 x 5 = 135) and a last tile that is mostly empty."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RK, SK = "conv_sk16<rk16 64x64>", "conv_sk16<64x64>"
STEPS = [5, 7, 5, 1, 3, 5]              # steps per stream and call: 1 = no shared row, the kernel declines; 3 with K 11 does not fit its LDS
SLOPE = float(np.float32(0.1))


def _eligible(t, k, dil, streams):
    """The shape rule of conv_rk16_eligible for the layers below (stride 1, whole 64-channel blocks): every staged row used twice at least,
    the rows of the streams of one 64-column tile within two 32 KiB buffers of 144-byte rows."""
    rps = (k - 1) * dil + t
    per_tile = min((t - 1 + 63) // t + 1, streams)
    return 2 * rps <= t * k and rps * per_tile <= 65536 // (2 * 144)


def _act64(v, act):
    return {None: lambda u: u, "ELU": F.elu, "LeakyReLU": lambda u: F.leaky_relu(u, SLOPE)}[act](v)


@pytest.fixture
def options():
    from audiodec_amd import native
    native.set_option("gv16_max_columns", 0)
    native.set_option("conv_rk16", 2)
    yield native
    native.set_option("conv_rk16", 1)
    native.set_option("gv16_max_columns", 32)


def _layer(cls, cin, cout, k, dil, groups, w, bias, act, B):
    from audiodec_amd import native
    m = cls(cin, cout, k, 1, dil, groups, True, device=DEV, batch=B, max_len=max(STEPS)).load(w, bias)
    m.set_activation(act, SLOPE)
    m.impl = native.IMPL_SPLIT16_SK
    return m


def _rep_class():
    from audiodec_amd import layers
    from audiodec_amd.native import ConvDesc

    class Rep(layers.CausalConv1d):
        """MultiGroupConv1d's x.repeat(1, groups, 1) (multi_fusion.py:133-141): every group reads the first cin_g channels of the ring
        (group input stride 0) -- CausalConv1d.inference with that one field changed."""

        def inference(self, x, residual=None):
            L = self._push(x)
            d = ConvDesc()
            d.cin_g, d.cout_g, d.groups = self.in_channels // self.groups, self.out_channels // self.groups, self.groups
            d.taps, d.stride, d.dilation, d.hist = self.kernel_size, 1, self.dilation, self.hist
            d.up, d.cout_real = 1, self.out_channels
            d.in_group_stride, d.res_group_stride = 0, d.cout_g
            out = self._run(d, L, L, self.out_channels, residual)
            self.cursor = (self.cursor + L) % self.rows
            return out.transpose(1, 2)

    return Rep


@pytest.mark.parametrize("cin_g,cout_g,groups,rep,k,res,act,B", [
    (256, 256, 3, False, 11, True, "LeakyReLU", 14),        # the vocoder's stage-0 shape; 70 columns: the second tile holds 6
    (128, 64, 1, False, 7, False, "ELU", 13),               # one m-tile; 65 columns: one column in the last tile
    (128, 64, 3, True, 11, True, "LeakyReLU", 27),          # x.repeat form; three n-tiles, the middle one starts and ends inside a stream
    (256, 64, 1, False, 7, True, None, 1),                  # one stream: a single tile of 5 / 7 / 3 columns
    (128, 256, 3, False, 7, False, "LeakyReLU", 27),
])
def test_rows_once_kernel_against_fp64_and_stream_k(gpu, options, cin_g, cout_g, groups, rep, k, res, act, B):
    """Six calls of 5, 7, 5, 1, 3, 5 steps (17- / 13-row rings: every ring wraps), one stream reset to silence half-way.  Where the call
    is eligible describe names conv_rk16 and the error against fp64 is at most twice the stream-K launch's on the same operands (both
    add the same exact products, in another order of f32 additions); elsewhere the stream-K kernel runs and the next eligible call
    continues from the ring it left.  A second module fed the same calls is bit-identical."""
    from audiodec_amd import layers
    native = options
    cin, cout = cin_g * groups, cout_g * groups
    g = torch.Generator().manual_seed(1000 * cin_g + 10 * k + B)
    w = torch.randn(cout, cin_g, k, generator=g) / (cin_g * k) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    cls = _rep_class() if rep else layers.CausalConv1d
    mods = {key: _layer(cls, cin, cout, k, 1, groups, w, bias, act, B) for key in ("rk", "rk2", "sk")}
    span = k - 1
    hist = torch.zeros(B, cin, span, dtype=torch.float64)
    w64, b64 = w.double(), bias.double()
    err = {"rk": 0.0, "sk": 0.0}
    ran = set()
    for call, t in enumerate(STEPS):
        if call == 3:                                        # one stream starts over: its history rows are zero (reset_buffer for that stream)
            hist[B - 1] = 0
            for m in mods.values():
                m.ring[B - 1].zero_()
        x = torch.randn(B, cin, t, generator=g)
        r = torch.randn(B, cout, t, generator=g) if res else None
        win = torch.cat([hist, x.double()], 2)
        a64 = _act64(win, act)
        if rep:
            a64 = a64[:, :cin_g].repeat(1, groups, 1)
        ref = F.conv1d(a64, w64, b64, dilation=1, groups=groups)
        if res:
            ref = ref + r.double()
        hist = win[:, :, -span:]
        y = {}
        for key, m in mods.items():
            native.set_option("conv_rk16", 0 if key == "sk" else 2)
            y[key] = m.inference(x.to(DEV), None if r is None else r.to(DEV))
        want = RK if _eligible(t, k, 1, B) else SK
        assert mods["rk"].last_kernel == want and mods["rk2"].last_kernel == want, (call, t, mods["rk"].last_kernel)
        assert mods["sk"].last_kernel == SK, (call, t, mods["sk"].last_kernel)
        ran.add(want)
        assert torch.equal(y["rk"], y["rk2"]), (call, t)
        e = {key: float((y[key].cpu().double() - ref).abs().max()) for key in ("rk", "sk")}
        assert e["rk"] < 2e-5 and e["sk"] < 2e-5, (call, t, e)
        if want == RK:
            err = {key: max(err[key], e[key]) for key in err}
    print(f"conv_rk16 cin_g={cin_g} cout_g={cout_g} groups={groups} K={k} B={B}: max|err| vs fp64  rk16 {err['rk']:.3e}  stream-K {err['sk']:.3e}")
    assert ran == {RK, SK}, ran
    assert err["rk"] <= 2.0 * err["sk"], err
    assert native.device_flags() == 0


def _two_conv_program(shadow, B, seed):
    """ring write -> conv a (128 -> 128, K 7) -> conv b (128 -> 128, K 11) -> out.  Lowered with shadow rings, the ring between the two
    convs has one: conv a stages from an f32 ring, conv b from a shadow; lowered without, both stage from f32 rings."""
    from audiodec_amd import arch, program
    from audiodec_amd.native import ACT_LEAKY
    C = 128
    specs = [arch.ConvSpec("a", "conv", C, C, 7), arch.ConvSpec("b", "conv", C, C, 11)]
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for s in specs:
        sd[s.wkey("weight")] = torch.randn(C, C, s.k, generator=g) / (C * s.k) ** 0.5
        sd[s.wkey("bias")] = torch.randn(C, generator=g) * 0.1
    old = program.SHADOW_RINGS
    program.SHADOW_RINGS = shadow
    try:
        b = program.Builder(sd, specs, split16=True)
        rx = b.ring(C, 0, 1)
        b.ring_write(rx, 0)
        mid = b.ring(C, 0, 1)
        b.conv("a", rx, mid, ACT_LEAKY, SLOPE)
        out = b.ring(C, 0, 1, external=1)
        b.conv("b", mid, out, ACT_LEAKY, SLOPE)
        pr = program.HipProgram(b, B, max(STEPS), DEV)
    finally:
        program.SHADOW_RINGS = old
    return pr


def test_shadow_and_f32_input_put_the_same_bits_in_lds(gpu, options):
    """The same two-conv program lowered with and without shadow rings, the calls of the test above (a per-stream reset in the middle):
    the outputs are equal bit for bit whether conv b stages 16-byte shadow pieces or converts f32 rows, the eligible calls are named
    conv_rk16 on both sides, and against the stream-K launches (option 0) the outputs agree to f32 round-off."""
    native = options
    B, C = 13, 128
    sh, pl = _two_conv_program(True, B, 5), _two_conv_program(False, B, 5)
    assert sum(1 for i in range(sh.n_ops) if sh._ops[i].in_shadow) == 1 and sum(1 for i in range(sh.n_ops) if sh._ops[i].out_shadow) == 1
    assert not any(pl._ops[i].in_shadow or pl._ops[i].out_shadow for i in range(pl.n_ops))
    sk = _two_conv_program(True, B, 5)
    g = torch.Generator().manual_seed(77)
    for call, t in enumerate(STEPS):
        if call == 3:
            for pr in (sh, pl, sk):
                pr.restore_stream_state(B - 1, None)
        for pr in (sh, pl):
            names = [pr.describe_op(i, t) for i in range(pr.n_ops)]
            assert names[1] == (RK if _eligible(t, 7, 1, B) else SK) and names[2] == (RK if _eligible(t, 11, 1, B) else SK), (t, names)
        x = torch.randn(B, t, C, generator=g).to(DEV)
        outs = []
        for pr in (sh, pl, sk):
            native.set_option("conv_rk16", 0 if pr is sk else 2)
            y = torch.empty(B, t, C, device=DEV)
            pr.step(t, (x, y))
            outs.append(y)
        native.set_option("conv_rk16", 2)
        assert torch.equal(outs[0], outs[1]), (call, t, float((outs[0] - outs[1]).abs().max()))
        assert float((outs[0] - outs[2]).abs().max()) < 2e-5, (call, t)
    assert sh.flags() == 0 and pl.flags() == 0 and sk.flags() == 0
    assert native.device_flags() == 0
