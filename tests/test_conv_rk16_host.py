"""CPU: which split-f16 stream-K-family launch a conv gets (csrc/conv_rk16.hip conv_rk16_preferred, csrc/conv_mfma.hip launch_conv_sk16),
read through adk_causal_conv_describe.  Host logic only: the pointers are stand-ins, nothing is launched."""
import ctypes as C

import pytest

RK, SK = "conv_sk16<rk16 64x64>", "conv_sk16<64x64>"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


def _describe(lib, cin_g, cout_g, groups, k, dil, t, B, gstride=None, max_len=None):
    from audiodec_amd import native
    from audiodec_amd.native import ConvDesc, RingView
    hist = (k - 1) * dil
    rows = hist + (max_len or t)
    d = ConvDesc()
    d.cin_g, d.cout_g, d.groups, d.taps, d.stride, d.dilation, d.hist = cin_g, cout_g, groups, k, 1, dil, hist
    d.up, d.cout_real = 1, cout_g * groups
    d.in_group_stride, d.res_group_stride = (cin_g if gstride is None else gstride), cout_g
    d.act_in, d.act_in_slope, d.act_out = native.ACT_LEAKY, 0.1, native.ACT_NONE
    d.w, d.w_frag, d.bias = None, 0x10000, None            # 16-byte aligned stand-ins: only geometry and alignment are looked at

    def view(base, r, ch, cur):
        v = RingView()
        v.base, v.rows, v.channels, v.cursor, v.ch_off = base, r, ch, cur, 0
        return v
    buf = C.create_string_buffer(64)
    rc = lib.adk_causal_conv_describe(C.byref(d), view(0x20000, rows, cin_g * groups, hist), view(0x30000, t, cout_g * groups, 0),
                                      view(None, 0, 0, 0), B, t, native.IMPL_SPLIT16_SK, buf, 64)
    assert rc == 0, lib.adk_last_error()
    return buf.value.decode()


def test_which_launches_the_rows_once_kernel_takes(lib, monkeypatch):
    from audiodec_amd import native
    monkeypatch.delenv("ADK_CONV_RK16", raising=False)
    try:
        native.set_option("conv_rk16", 1)
        # the vocoder's first stage at 256 streams, one frame (5 steps) per call: 3 groups x 4 m-tiles x 20 n-tiles = 240 tiles
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 256) == RK
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 256, gstride=0) == SK          # the x.repeat form: by default the stream-K kernel's (option 2 below)
        assert _describe(lib, 128, 128, 3, 11, 1, 25, 224) == "conv_sk16<128x64>"    # where the stream-K launch picks 128-row tiles it keeps them
        assert _describe(lib, 256, 256, 3, 11, 3, 5, 256) == SK                     # dilation 3: 35 rows for 55 (step, tap) pairs, 14 streams do not fit
        assert _describe(lib, 256, 256, 3, 11, 5, 5, 256) == SK                     # dilation 5: no row is shared
        assert _describe(lib, 256, 256, 3, 11, 1, 1, 256, max_len=5) == SK          # one step per stream: no row is shared
        assert _describe(lib, 256, 256, 3, 11, 1, 3, 256, max_len=5) == SK          # 3 steps: 22 streams x 13 rows per tile exceed the LDS buffers
        assert _describe(lib, 256, 256, 3, 11, 1, 7, 256, max_len=7) == RK
        assert _describe(lib, 256, 256, 3, 7, 1, 3, 512, max_len=5) == RK           # K 7 at 3 steps: 22 x 9 rows fit (512 streams: 288 tiles)
        assert _describe(lib, 64, 64, 3, 11, 1, 5, 256) == SK                       # narrow groups: not this kernel's
        assert _describe(lib, 192, 256, 3, 11, 1, 5, 256) == RK and _describe(lib, 160, 256, 3, 11, 1, 5, 256) == SK     # whole 64-channel blocks
        assert _describe(lib, 256, 96, 3, 11, 1, 5, 256).startswith("conv_sk16<") and "rk16" not in _describe(lib, 256, 96, 3, 11, 1, 5, 256)
        # launches that do not fill the chip stay on the stream-K kernel (encoder block 3 at 256 streams: 80 tiles) unless the option is 2
        assert _describe(lib, 256, 256, 1, 7, 1, 5, 256) == SK
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 64) == SK
        native.set_option("conv_rk16", 2)
        assert _describe(lib, 256, 256, 1, 7, 1, 5, 256) == RK and _describe(lib, 256, 256, 3, 11, 1, 5, 64) == RK
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 256, gstride=0) == RK and _describe(lib, 128, 128, 3, 11, 1, 25, 224) == "conv_sk16<128x64>"
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 6) == "conv_gv16<32>"          # few columns: the GEMV-shaped kernel comes first
        assert _describe(lib, 256, 256, 3, 11, 1, 1, 256, max_len=5) == SK
        native.set_option("conv_rk16", 0)
        assert _describe(lib, 256, 256, 3, 11, 1, 5, 256) == SK
    finally:
        native.set_option("conv_rk16", 1)
