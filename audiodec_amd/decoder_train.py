"""The symmetric decoder as a trainable module on the HIP path (adk_convtr_wgrad: csrc/dec_wgrad.hip; adk_conv_wgrad for the
stride-1 convs: csrc/enc_grad.hip; adk_dec_conv, adk_dec_convtr and their ``_grad`` calls: csrc/dec_grad.hip).

Stage 1 of the reference's autoencoder flow (``trainer/autoencoder.py:84-112``) trains encoder, projector, quantizer and decoder
on the metric loss; the second half of the 'efficient' paradigm freezes everything but the decoder and adds the GAN terms, which
reach ``y_hat`` through the discriminators' backward to their input.  ``TrainableEncoder`` is the first half of that step,
``TrainableDecoder`` the second: the gradient that the losses leave at ``y_hat`` goes to the decoder's own parameters and, when
``zq`` requires grad, on to ``zq``.

``TrainableDecoder`` mirrors the reference ``Generator``'s ``decoder`` (``models/autoencoder/modules/decoder.py:79-138``, 'causal'
mode, ELU) as one ``torch.nn.Module`` whose parameters carry the generator's state-dict keys (``decoder.*``) in the reference's
layout.  Its forward is the non-streaming ``Decoder.forward`` on (B, code_dim, T) tensors with ``FrozenDecoder``'s calls: one HIP
call per conv, exact f32, conv2 on the direct kernel.  With grad enabled, conv1, conv2, every transposed conv and every residual
unit (its two convs and its skip) is a once-differentiable ``torch.autograd.Function`` whose backward returns dx, dW and db from
the native calls and skips what ``needs_input_grad`` does not ask for.  What is kept until backward is the pre-activation input of
every conv.  Forward and gradients are bitwise reproducible; without grad the output is bitwise ``FrozenDecoder``'s.

The GEMM kernels read re-packed weights; the packings are rebuilt on the device, under ``no_grad``, when a parameter's version
counter has moved (an optimizer step, ``load_state_dict``), not on every call.

The streaming generators, their programs, rings, guard and split-f16 kernels are not used and not touched.
"""
import ctypes as C
import math

import torch

from . import arch, native
from .decoder_grad import (ACT_ELU, ACT_NONE, DIRECT_MAX_COUT, IMPL_DIRECT, IMPL_GEMM, _upstream, pack_conv, pack_conv_grad,
                           pack_convtr, pack_convtr_grad)
from .encoder_grad import _Workspace, wgrad_plan
from .loss_common import _ptr, _settled
from .stream_generator import _AE_DEFAULTS, _merge

_OTHERS = ("encoder.", "projector.", "quantizer.")


def convtr_wgrad_plan(n_items, c_in, t, c_out, kernel, stride):
    """(workspace bytes, slices) of adk_convtr_wgrad for a shape; host only."""
    ws, s = C.c_int64(0), C.c_int32(0)
    native.check(native.lib().adk_convtr_wgrad_plan(n_items, c_in, t, c_out, kernel, stride, C.byref(ws), C.byref(s)),
                 "adk_convtr_wgrad_plan")
    return int(ws.value), int(s.value)


class _Layer:
    """One conv of the decoder: its spec, its input activation, and the packed forms of its weight."""

    def __init__(self, spec, act, alpha):
        self.spec, self.act, self.alpha = spec, act, float(alpha)
        self.transposed = spec.kind == "convT"
        self.impl = IMPL_DIRECT if not self.transposed and spec.cout <= DIRECT_MAX_COUT else IMPL_GEMM
        self._key = None
        self._wf = self._wg = None

    def packs(self, w):
        """(forward packing, backward-data packing) of parameter w, rebuilt when w has changed since the last call."""
        key = (w._version, w.data_ptr(), w.device)
        if key != self._key:
            with torch.no_grad():
                wd = w.detach()
                if self.transposed:
                    self._wf, self._wg = pack_convtr(wd, self.spec.stride), pack_convtr_grad(wd, self.spec.stride)
                else:
                    self._wf = wd.contiguous().clone() if self.impl == IMPL_DIRECT else pack_conv(wd)
                    self._wg = pack_conv_grad(wd)
            self._key = key
        return self._wf, self._wg

    def out_shape(self, x_shape):
        b, _, t = x_shape
        return b, self.spec.cout, t * self.spec.stride

    def forward(self, x, wf, bias, res=None):
        s, lib = self.spec, native.lib()
        y = torch.empty(*self.out_shape(x.shape), dtype=torch.float32, device=x.device)
        b, _, t = x.shape
        st = native.current_stream(x.device)
        if self.transposed:
            native.check(lib.adk_dec_convtr(_ptr(x), _ptr(wf), _ptr(bias), _ptr(y), b, s.cin, t, s.cout, s.k, s.stride, self.act,
                                            self.alpha, st), "adk_dec_convtr")
        else:
            native.check(lib.adk_dec_conv(_ptr(x), _ptr(wf), _ptr(bias), _ptr(res), _ptr(y), b, s.cin, t, s.cout, s.k, s.dilation,
                                          self.act, self.alpha, self.impl, st), "adk_dec_conv")
        return y

    def grad_input(self, dy, x, x_shape, wg, dres=None):
        """dy of the output's shape, x the saved input [+ dres of x's shape] -> dx."""
        s, lib = self.spec, native.lib()
        dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
        b, _, t = x_shape
        st = native.current_stream(dy.device)
        xa = x if self.act != ACT_NONE else None
        if self.transposed:
            native.check(lib.adk_dec_convtr_grad(_ptr(dy), _ptr(xa), _ptr(wg), _ptr(dx), b, s.cin, t, s.cout, s.k, s.stride,
                                                 self.act, self.alpha, st), "adk_dec_convtr_grad")
        else:
            native.check(lib.adk_dec_conv_grad(_ptr(dy), _ptr(xa), _ptr(wg), _ptr(dres), _ptr(dx), b, s.cin, t, s.cout, s.k,
                                               s.dilation, self.act, self.alpha, st), "adk_dec_conv_grad")
        return dx

    def grad_weight(self, dy, x, workspace, want_bias):
        """dy of the output's shape, x the saved input -> (dW in the reference's layout, db or None)."""
        s, lib = self.spec, native.lib()
        b, _, t = x.shape
        st = native.current_stream(dy.device)
        db = torch.empty(s.cout, dtype=torch.float32, device=dy.device) if want_bias else None
        if self.transposed:
            n_bytes, _ = convtr_wgrad_plan(b, s.cin, t, s.cout, s.k, s.stride)
            ws = workspace.get(n_bytes, dy.device)
            dw = torch.empty(s.cin, s.cout, s.k, dtype=torch.float32, device=dy.device)
            native.check(lib.adk_convtr_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), b, s.cin, t, s.cout, s.k, s.stride,
                                              self.act, self.alpha, st), "adk_convtr_wgrad")
        else:
            n_bytes, _ = wgrad_plan(b, s.cin, t, s.cout, s.k, s.dilation, 1)
            ws = workspace.get(n_bytes, dy.device)
            dw = torch.empty(s.cout, s.cin, s.k, dtype=torch.float32, device=dy.device)
            native.check(lib.adk_conv_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), b, s.cin, t, s.cout, s.k, s.dilation, 1,
                                            self.act, self.alpha, st), "adk_conv_wgrad")
        return dw, db


class _ConvFn(torch.autograd.Function):
    """One conv or transposed conv (with its input activation): backward to its input, its weight and its bias."""

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


class TrainableDecoder(torch.nn.Module):
    """``Generator(...).decoder`` of the reference as a trainable module: the constructor takes the generator's parameters (the
    encoder's, the projector's and the quantizer's are accepted and not used).  ``forward(zq)``: (B, code_dim, T) ->
    (B, output_channels, T * hop)."""

    def __init__(self, device=None, **generator_params):
        super().__init__()
        generator_params = dict(generator_params)
        kernel_size = generator_params.pop("kernel_size", 7)                       # Decoder's own argument; the generator has none
        p = _merge(_AE_DEFAULTS, generator_params, "TrainableDecoder")
        if p["codec"] != "audiodec":
            raise NotImplementedError(f"codec {p['codec']!r}: TrainableDecoder implements Decoder only, not ActivateDecoder")
        if p["use_weight_norm"]:
            raise NotImplementedError("use_weight_norm=True: TrainableDecoder has no weight_g / weight_v gradients")
        if p["mode"] != "causal":
            raise NotImplementedError(f"mode {p['mode']!r}: TrainableDecoder implements the causal decoder only")
        if p["nonlinear_activation"] != "ELU":
            raise NotImplementedError(f"nonlinear_activation {p['nonlinear_activation']!r}: TrainableDecoder implements ELU only")
        unknown = set(p["nonlinear_activation_params"] or {}) - {"alpha"}
        if unknown:
            raise NotImplementedError(f"nonlinear_activation_params {sorted(unknown)}: only ELU's alpha is implemented")
        if kernel_size != 7:
            raise NotImplementedError("kernel_size: the reference's residual units and this class are written for 7")
        if len(p["dec_ratios"]) != len(p["dec_strides"]):
            raise ValueError("dec_ratios and dec_strides must have the same length")
        if min(p["output_channels"], p["decode_channels"], p["code_dim"], *p["dec_ratios"], *p["dec_strides"]) < 1:
            raise ValueError("output_channels, decode_channels, code_dim, dec_ratios and dec_strides must be positive")
        self.params = p
        self.alpha = float((p["nonlinear_activation_params"] or {}).get("alpha", 1.0))
        self.code_dim, self.output_channels = int(p["code_dim"]), int(p["output_channels"])
        self.hop = 1
        for s in p["dec_strides"]:
            self.hop *= int(s)
        self._specs = arch.autoencoder_decoder_convs(p)
        # the input activation of each conv: the residual units' two convs have one, nothing else (decoder.py, residual_unit.py:45-48)
        self._layers = [_Layer(s, ACT_ELU if ".res_units." in s.name else ACT_NONE, self.alpha) for s in self._specs]
        self._workspace = _Workspace()
        for s in self._specs:
            w = torch.empty(*s.wshape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5))                      # torch's Conv1d / ConvTranspose1d.reset_parameters
            self._register(s.wkey("weight"), w)
            if s.bias:
                fan_in = w.shape[1] * w.shape[2]                                   # torch's fan-in: dim 1 x the kernel, both kinds
                bound = 1.0 / math.sqrt(fan_in)
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
        """The decoder of an ``AutoEncoderStreamGenerator`` with copies of its loaded weights; the generator is only read."""
        if gen._sd is None:
            raise RuntimeError("from_generator: the generator has no weights loaded (call load_state_dict first)")
        dec = cls(**gen.params)
        dec.load_state_dict(gen._sd)
        dev = device if device is not None else gen._device
        return dec.to(native.require_gpu(dev)) if dev is not None else dec

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The generator's state dict (``encoder.*``, ``projector.*``, ``quantizer.*`` and the streaming ``*.pad_buffer`` entries are
        ignored) or the decoder's own keys, without the ``decoder.`` prefix."""
        own = {k: v for k, v in state_dict.items() if not (k.startswith(_OTHERS) or k.endswith(".pad_buffer"))}
        if own and not any(k.startswith("decoder.") for k in own):
            own = {f"decoder.{k}": v for k, v in own.items()}
        return super().load_state_dict(own, strict=strict, **kwargs)

    def saved_floats(self, batch, frames):
        """Floats a differentiable pass keeps until backward for a (batch, code_dim, frames) input: the pre-activation input of
        every conv."""
        n, t = 0, frames
        for s in self._specs:
            n += batch * s.cin * t
            t *= s.stride if s.kind == "convT" else 1
        return n

    def forward(self, zq):
        if not isinstance(zq, torch.Tensor) or zq.dim() != 3 or zq.shape[1] != self.code_dim:
            raise ValueError(f"expected a (B, {self.code_dim}, T) input, got {tuple(getattr(zq, 'shape', ()))}")
        if zq.shape[0] == 0 or zq.shape[2] == 0:
            raise ValueError(f"empty input {tuple(zq.shape)}")
        L, P = self._layers, [(self._param(s.wkey("weight")), self._param(s.wkey("bias")) if s.bias else None) for s in self._specs]
        dev = P[0][0].device
        if any(w.dtype != torch.float32 or w.device != dev for w, _ in P):
            raise TypeError("TrainableDecoder computes in float32 with every parameter on one device")
        native.require_gpu(dev)
        zq = _settled(zq)
        grad = torch.is_grad_enabled() and (zq.requires_grad or any(p.requires_grad for p in self.parameters()))
        x = zq.to(device=dev, dtype=torch.float32).contiguous()
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
                h = conv(h, i)                                 # the block's transposed conv
                i += 1
        return conv(h, len(L) - 1)
