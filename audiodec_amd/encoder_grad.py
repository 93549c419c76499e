"""The encoder and projector as a trainable module on the HIP path (adk_enc_down, adk_enc_down_grad, adk_conv_wgrad:
csrc/enc_grad.hip; adk_dec_conv and adk_dec_conv_grad for the stride-1 layers: csrc/dec_grad.hip).

The reference's denoising flow (``trainer/denoise.py``) freezes the quantizer and the decoder and trains the encoder and the
projector.  ``decoder_grad.FrozenDecoder`` and ``quantize_st`` carry the gradient of the metric loss back to the latent ``z``;
``TrainableEncoder`` takes it from there to its own parameters (and to ``x`` when that requires grad).

``TrainableEncoder`` mirrors the reference ``Generator``'s ``encoder`` (``models/autoencoder/modules/encoder.py:84-142``, 'causal'
mode, ELU) and ``projector`` (``modules/projector.py:20-50``, 'conv1d') as one ``torch.nn.Module`` whose parameters carry the
reference's state-dict keys in the reference's layout.  Its forward is the non-streaming ``projector(encoder(x))`` on (B, C, T)
tensors: one HIP call per conv, exact f32.  With grad enabled, the first conv, every strided conv, the projector and every residual
unit (its two convs and its skip) is a once-differentiable ``torch.autograd.Function`` whose backward returns dx, dW and db from the
native calls and skips what ``needs_input_grad`` does not ask for.  What is kept until backward is the pre-activation input of every
conv.  Forward and gradients are bitwise reproducible.

The GEMM kernels read re-packed weights; the packings are rebuilt on the device, under ``no_grad``, when a parameter's version
counter has moved (an optimizer step, ``load_state_dict``), not on every call.

The streaming generators, their programs, rings, guard and split-f16 kernels are not used and not touched.
"""
import ctypes as C
import math

import torch

from . import arch, native
from .decoder_grad import ACT_ELU, ACT_NONE, IMPL_GEMM, _upstream, pack_conv, pack_conv_grad
from .loss_common import _ptr, _settled
from .stream_generator import _AE_DEFAULTS, _merge


def out_length(t, stride):
    """Output length of a causal conv with left padding (k - 1) d: (t - 1) // stride + 1."""
    return (t - 1) // stride + 1


def pack_down_grad(w, stride):
    """Strided Conv1d weight (C_out, C_in, 2s) -> the backward-data GEMMs' [r][kk = 2*co + tap][ci], one per phase r = v % s of the
    input index v: tap 0 is W[co][ci][j0], j0 = (r + s - 1) % s, which reads dy[v // s + (2 if r else 1)]; tap 1 is W[co][ci][j0 + s],
    which reads the output before that one."""
    co, ci, k = w.shape
    if k != 2 * stride:
        raise ValueError(f"strided conv: kernel {k} is not 2 * stride = {2 * stride}")
    j0 = (torch.arange(stride, device=w.device) + stride - 1) % stride
    taps = torch.stack([j0, j0 + stride], 1)                               # (s, 2)
    return w[:, :, taps].permute(2, 0, 3, 1).reshape(stride, 2 * co, ci).contiguous()


def wgrad_plan(n_items, c_in, t, c_out, kernel, dilation=1, stride=1):
    """(workspace bytes, slices) of adk_conv_wgrad for a shape; host only."""
    ws, s = C.c_int64(0), C.c_int32(0)
    native.check(native.lib().adk_conv_wgrad_plan(n_items, c_in, t, c_out, kernel, dilation, stride, C.byref(ws), C.byref(s)),
                 "adk_conv_wgrad_plan")
    return int(ws.value), int(s.value)


class _Workspace:
    """The weight gradient's partial tiles: one buffer per device, grown to the largest plan seen.  Launches that share it are
    ordered on the stream they run on."""

    def __init__(self):
        self._buf = {}

    def get(self, n_bytes, dev):
        buf = self._buf.get(dev)
        if buf is None or buf.numel() * 4 < n_bytes:
            buf = self._buf[dev] = torch.empty(max(1, (n_bytes + 3) // 4), dtype=torch.float32, device=dev)
        return buf


class _Layer:
    """One conv of the encoder: its spec, its input activation, and the packed forms of its weight."""

    def __init__(self, spec, act, alpha):
        self.spec, self.act, self.alpha = spec, act, float(alpha)
        self._key = None
        self._wf = self._wg = None

    def packs(self, w):
        """(forward packing, backward-data packing) of parameter w, rebuilt when w has changed since the last call."""
        key = (w._version, w.data_ptr(), w.device)
        if key != self._key:
            with torch.no_grad():
                wd = w.detach()
                self._wf = pack_conv(wd)
                self._wg = pack_down_grad(wd, self.spec.stride) if self.spec.stride > 1 else pack_conv_grad(wd)
            self._key = key
        return self._wf, self._wg

    def out_shape(self, x_shape):
        b, _, t = x_shape
        return b, self.spec.cout, out_length(t, self.spec.stride)

    def forward(self, x, wf, bias, res=None):
        s, lib = self.spec, native.lib()
        y = torch.empty(*self.out_shape(x.shape), dtype=torch.float32, device=x.device)
        b, _, t = x.shape
        st = native.current_stream(x.device)
        if s.stride > 1:
            native.check(lib.adk_enc_down(_ptr(x), _ptr(wf), _ptr(bias), _ptr(y), b, s.cin, t, s.cout, s.k, s.stride, st),
                         "adk_enc_down")
        else:
            native.check(lib.adk_dec_conv(_ptr(x), _ptr(wf), _ptr(bias), _ptr(res), _ptr(y), b, s.cin, t, s.cout, s.k, s.dilation,
                                          self.act, self.alpha, IMPL_GEMM, st), "adk_dec_conv")
        return y

    def grad_input(self, dy, x, x_shape, wg, dres=None):
        """dy of the output's shape, x the saved input [+ dres of x's shape] -> dx."""
        s, lib = self.spec, native.lib()
        dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
        b, _, t = x_shape
        st = native.current_stream(dy.device)
        if s.stride > 1:
            native.check(lib.adk_enc_down_grad(_ptr(dy), _ptr(wg), _ptr(dx), b, s.cin, t, s.cout, s.k, s.stride, st),
                         "adk_enc_down_grad")
        else:
            native.check(lib.adk_dec_conv_grad(_ptr(dy), _ptr(x if self.act != ACT_NONE else None), _ptr(wg), _ptr(dres), _ptr(dx),
                                               b, s.cin, t, s.cout, s.k, s.dilation, self.act, self.alpha, st), "adk_dec_conv_grad")
        return dx

    def grad_weight(self, dy, x, workspace, want_bias):
        """dy of the output's shape, x the saved input -> (dW in the reference's layout, db or None)."""
        s, lib = self.spec, native.lib()
        b, _, t = x.shape
        n_bytes, _ = wgrad_plan(b, s.cin, t, s.cout, s.k, s.dilation, s.stride)
        ws = workspace.get(n_bytes, dy.device)
        dw = torch.empty(s.cout, s.cin, s.k, dtype=torch.float32, device=dy.device)
        db = torch.empty(s.cout, dtype=torch.float32, device=dy.device) if want_bias else None
        native.check(lib.adk_conv_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), b, s.cin, t, s.cout, s.k, s.dilation,
                                        s.stride, self.act, self.alpha, native.current_stream(dy.device)), "adk_conv_wgrad")
        return dw, db


class _ConvFn(torch.autograd.Function):
    """One conv (with its input activation): backward to its input, its weight and its bias."""

    @staticmethod
    def forward(ctx, x, w, b, layer, workspace):
        wf, wg = layer.packs(w)
        ctx.layer, ctx.workspace, ctx.wg, ctx.x_shape = layer, workspace, wg, tuple(x.shape)
        ctx.save_for_backward(x)
        return layer.forward(x, wf, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dy = _upstream(dy)
        dx = ctx.layer.grad_input(dy, x, ctx.x_shape, ctx.wg) if need_x else None
        dw = db = None
        if need_w or need_b:
            dw, db = ctx.layer.grad_weight(dy, x, ctx.workspace, need_b)
        return dx, (dw if need_w else None), db, None, None


class _ResUnitFn(torch.autograd.Function):
    """One residual unit, x + conv2(a(conv1(a(x)))): the skip is conv2's epilogue going forward and conv1's going back."""

    @staticmethod
    def forward(ctx, x, w1, w2, conv1, conv2, workspace):
        (wf1, wg1), (wf2, wg2) = conv1.packs(w1), conv2.packs(w2)
        ctx.convs, ctx.workspace, ctx.wg, ctx.x_shape = (conv1, conv2), workspace, (wg1, wg2), tuple(x.shape)
        h = conv1.forward(x, wf1, None)
        ctx.save_for_backward(x, h)
        return conv2.forward(h, wf2, None, res=x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        conv1, conv2 = ctx.convs
        x, h = ctx.saved_tensors
        need_x, need_w1, need_w2 = ctx.needs_input_grad[:3]
        dy = _upstream(dy)
        dw1 = dw2 = dx = None
        if need_w2:
            dw2, _ = conv2.grad_weight(dy, h, ctx.workspace, False)
        if need_x or need_w1:
            dh = conv2.grad_input(dy, h, tuple(h.shape), ctx.wg[1])
            if need_w1:
                dw1, _ = conv1.grad_weight(dh, x, ctx.workspace, False)
            if need_x:
                dx = conv1.grad_input(dh, x, ctx.x_shape, ctx.wg[0], dres=dy)
        return dx, dw1, dw2, None, None, None


class TrainableEncoder(torch.nn.Module):
    """``Generator(...).encoder`` and ``.projector`` of the reference as one trainable module: the constructor takes the
    generator's parameters (the decoder's and the quantizer's are accepted and not used).  ``forward(x)``: (B, input_channels, T) ->
    z (B, code_dim, T_out), T_out the length after the four causal strided convs ((t - 1) // s + 1 each), for any T >= 1."""

    def __init__(self, device=None, **generator_params):
        super().__init__()
        p = _merge(_AE_DEFAULTS, generator_params, "TrainableEncoder")
        if p["codec"] != "audiodec":
            raise NotImplementedError(f"codec {p['codec']!r}: TrainableEncoder implements Encoder only, not ActivateEncoder")
        if p["use_weight_norm"]:
            raise NotImplementedError("use_weight_norm=True: TrainableEncoder has no weight_g / weight_v gradients")
        if p["mode"] != "causal":
            raise NotImplementedError(f"mode {p['mode']!r}: TrainableEncoder implements the causal encoder only")
        if p["nonlinear_activation"] != "ELU":
            raise NotImplementedError(f"nonlinear_activation {p['nonlinear_activation']!r}: TrainableEncoder implements ELU only")
        unknown = set(p["nonlinear_activation_params"] or {}) - {"alpha"}
        if unknown:
            raise NotImplementedError(f"nonlinear_activation_params {sorted(unknown)}: only ELU's alpha is implemented")
        if p["projector"] != "conv1d":
            raise NotImplementedError(f"projector {p['projector']!r}: TrainableEncoder implements the conv1d projector only")
        if len(p["enc_ratios"]) != len(p["enc_strides"]):
            raise ValueError("enc_ratios and enc_strides must have the same length")
        if min(p["input_channels"], p["encode_channels"], p["code_dim"], *p["enc_ratios"], *p["enc_strides"]) < 1:
            raise ValueError("input_channels, encode_channels, code_dim, enc_ratios and enc_strides must be positive")
        self.params = p
        self.alpha = float((p["nonlinear_activation_params"] or {}).get("alpha", 1.0))
        self.input_channels, self.code_dim = int(p["input_channels"]), int(p["code_dim"])
        self.hop = arch.hop_length(p)
        self._specs = arch.autoencoder_encoder_convs(p)
        # the input activation of each conv: the residual units' two convs have one, nothing else (encoder.py, residual_unit.py:45-48)
        self._layers = [_Layer(s, ACT_ELU if ".res_units." in s.name else ACT_NONE, self.alpha) for s in self._specs]
        self._workspace = _Workspace()
        for s in self._specs:
            w = torch.empty(*s.wshape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5))                      # torch.nn.Conv1d.reset_parameters
            self._register(s.wkey("weight"), w)
            if s.bias:
                bound = 1.0 / math.sqrt(s.cin * s.k)
                self._register(s.wkey("bias"), torch.empty(s.cout, dtype=torch.float32).uniform_(-bound, bound))
        if device is not None:
            self.to(native.require_gpu(device))

    def _register(self, key, value):
        """A parameter under the reference's dotted key: the modules along the path are plain containers."""
        *path, leaf = key.split(".")
        mod = self
        for name in path:
            if name not in mod._modules:
                mod.add_module(name, torch.nn.Module())
            mod = mod._modules[name]
        mod.register_parameter(leaf, torch.nn.Parameter(value))

    def _param(self, key):
        *path, leaf = key.split(".")
        mod = self
        for name in path:
            mod = mod._modules[name]
        return mod._parameters[leaf]

    @classmethod
    def from_generator(cls, gen, device=None):
        """The encoder and projector of an ``AutoEncoderStreamGenerator`` with copies of its loaded weights; the generator is only
        read."""
        if gen._sd is None:
            raise RuntimeError("from_generator: the generator has no weights loaded (call load_state_dict first)")
        enc = cls(**gen.params)
        enc.load_state_dict(gen._sd)
        dev = device if device is not None else gen._device
        return enc.to(native.require_gpu(dev)) if dev is not None else enc

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The generator's state dict: ``decoder.*``, ``quantizer.*`` and the streaming ``*.pad_buffer`` entries are ignored."""
        own = {k: v for k, v in state_dict.items()
               if not (k.startswith("decoder.") or k.startswith("quantizer.") or k.endswith(".pad_buffer"))}
        return super().load_state_dict(own, strict=strict, **kwargs)

    def saved_floats(self, batch, samples):
        """Floats a differentiable pass keeps until backward for a (batch, input_channels, samples) input: the pre-activation input
        of every conv."""
        n, t = 0, samples
        for s in self._specs:
            n += batch * s.cin * t
            t = out_length(t, s.stride)
        return n

    def out_frames(self, samples):
        t = samples
        for s in self._specs:
            t = out_length(t, s.stride)
        return t

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.input_channels:
            raise ValueError(f"expected a (B, {self.input_channels}, T) input, got {tuple(getattr(x, 'shape', ()))}")
        if x.shape[0] == 0 or x.shape[2] == 0:
            raise ValueError(f"empty input {tuple(x.shape)}")
        L, P = self._layers, [(self._param(s.wkey("weight")), self._param(s.wkey("bias")) if s.bias else None) for s in self._specs]
        dev = P[0][0].device
        if any(w.dtype != torch.float32 or w.device != dev for w, _ in P):
            raise TypeError("TrainableEncoder computes in float32 with every parameter on one device")
        native.require_gpu(dev)
        x = _settled(x)
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        ws = self._workspace
        if grad:
            conv = lambda h, i: _ConvFn.apply(h, P[i][0], P[i][1], L[i], ws)                                      # noqa: E731
            unit = lambda h, i: _ResUnitFn.apply(h, P[i][0], P[i + 1][0], L[i], L[i + 1], ws)                     # noqa: E731
        else:
            conv = lambda h, i: L[i].forward(h, L[i].packs(P[i][0])[0], P[i][1])                                  # noqa: E731
            unit = lambda h, i: L[i + 1].forward(L[i].forward(h, L[i].packs(P[i][0])[0], None),                   # noqa: E731
                                                 L[i + 1].packs(P[i + 1][0])[0], None, res=h)
        h = conv(x, 0)
        i = 1
        while i < len(L) - 1:
            if ".res_units." in L[i].spec.name:
                h = unit(h, i)
                i += 2
            else:
                h = conv(h, i)                                 # the block's strided conv
                i += 1
        return conv(h, len(L) - 1)
