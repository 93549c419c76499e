"""The HiFi-GAN vocoder as a trainable module on the HIP path (adk_voc_conv, adk_voc_convtr and their ``_grad`` calls:
csrc/dec_grad.hip; adk_voc_conv_wgrad: csrc/enc_grad.hip; adk_voc_convtr_wgrad: csrc/dec_wgrad.hip).

Stage 2 of the reference's flow (``trainer/vocoder.py:65-90``) freezes encoder, projector and quantizer and trains the HiFi-GAN
``Generator`` on ``zq``: the metric loss plus the adversarial and feature-matching terms, which reach ``y_`` through a
discriminator's backward to its input.  ``TrainableEncoder`` and ``TrainableDecoder`` cover the other two steps; this is the third.

``TrainableVocoder`` mirrors ``models/vocoder/HiFiGAN.py:28-161`` (LeakyReLU, ``MultiGroupConv1d`` or ``MultiReceptiveField``
blocks, with or without the additional convs) as one ``torch.nn.Module`` whose parameters carry the reference's state-dict keys:
``weight_g`` / ``weight_v`` / ``bias`` with weight norm, ``weight`` / ``bias`` without; ``mean`` and ``scale`` are buffers when the
model normalises its input.  Its forward is ``Generator.forward`` on (B, in_channels, T) tensors: one HIP call per conv, exact
f32, grouped convs as one launch, ``output_conv`` on the direct kernel.  With grad enabled every conv and every residual unit
(``x + convs2(a(convs1(a(x))))``, or ``x + convs1(a(x))`` without the additional convs) is a once-differentiable
``torch.autograd.Function`` whose backward returns dx, dW and db from the native calls and skips what ``needs_input_grad`` does not
ask for.  What is parameter-sized or elementwise stays torch and is differentiated by autograd: the weight-norm composition
``w = v g / ||v||`` (through which dW reaches ``weight_g`` and ``weight_v``), ``x.repeat(1, G, 1)``, the MRF average, the input
normalisation and the final ``tanh``.  Forward and gradients are bitwise reproducible.

The GEMM kernels read re-packed weights; the packings are rebuilt on the device, under ``no_grad``, when a parameter's version
counter, storage or device has changed (an optimizer step, ``load_state_dict``), not on every call.

The streaming generators, their programs, rings, guard and split-f16 kernels are not used and not touched.
"""
import ctypes as C
import math

import torch

from . import arch, native
from .decoder_grad import DIRECT_MAX_COUT, IMPL_DIRECT, IMPL_GEMM, _upstream, pack_convtr, pack_convtr_grad
from .decoder_train import TrainableDecoder, convtr_wgrad_plan
from .encoder_grad import _Workspace
from .loss_common import _ptr, _settled
from .stream_generator import _HG_DEFAULTS, _merge

ACT_NONE, ACT_LEAKY = native.ACT_NONE, native.ACT_LEAKY
OUTPUT_SLOPE = 0.01                     # nn.LeakyReLU()'s default, in front of output_conv (HiFiGAN.py:116)


def pack_conv(w, groups):
    """Conv1d weight (C_out, C_in/G, k) -> the forward GEMMs' [g][kk = ci*k + j][co of the group]."""
    co, cig, k = w.shape
    return w.reshape(groups, co // groups, cig * k).transpose(1, 2).contiguous()


def pack_conv_grad(w, groups):
    """Conv1d weight (C_out, C_in/G, k) -> the backward-data GEMMs' [g][kk = co*k + j][ci of the group]."""
    co, cig, k = w.shape
    return w.reshape(groups, co // groups, cig, k).permute(0, 1, 3, 2).reshape(groups, (co // groups) * k, cig).contiguous()


def conv_wgrad_plan(n_items, c_in, t, c_out, kernel, dilation=1, groups=1):
    """(workspace bytes, slices) of adk_voc_conv_wgrad for a shape; host only."""
    ws, s = C.c_int64(0), C.c_int32(0)
    native.check(native.lib().adk_voc_conv_wgrad_plan(n_items, c_in, t, c_out, kernel, dilation, groups, C.byref(ws), C.byref(s)),
                 "adk_voc_conv_wgrad_plan")
    return int(ws.value), int(s.value)


def weight_norm(g, v):
    """torch.nn.utils.weight_norm's composition over dim 0: w = v g / ||v||, the norm per slice v[i]."""
    return v * (g / torch.linalg.vector_norm(v, 2, dim=(1, 2), keepdim=True))


class _Layer:
    """One conv of the vocoder: its spec, its input activation, and the packed forms of its weight."""

    def __init__(self, spec, act, alpha):
        self.spec, self.act, self.alpha = spec, act, float(alpha)
        self.transposed = spec.kind == "convT"
        self.impl = IMPL_DIRECT if not self.transposed and spec.groups == 1 and spec.cout <= DIRECT_MAX_COUT else IMPL_GEMM
        self._key = None
        self.wf = self.wg = None        # forward packing, backward-data packing

    def stale(self, key):
        return key != self._key

    def repack(self, key, w):
        """The packings of the composed weight w (the reference's layout), kept under the parameters' key."""
        with torch.no_grad():
            wd, s = w.detach(), self.spec
            if self.transposed:
                self.wf, self.wg = pack_convtr(wd, s.stride), pack_convtr_grad(wd, s.stride)
            else:
                self.wf = wd.contiguous().clone() if self.impl == IMPL_DIRECT else pack_conv(wd, s.groups)
                self.wg = pack_conv_grad(wd, s.groups)
        self._key = key

    def forward(self, x, bias, res=None):
        s, lib = self.spec, native.lib()
        b, _, t = x.shape
        y = torch.empty(b, s.cout, t * s.stride, dtype=torch.float32, device=x.device)
        st = native.current_stream(x.device)
        if self.transposed:
            native.check(lib.adk_voc_convtr(_ptr(x), _ptr(self.wf), _ptr(bias), _ptr(y), b, s.cin, t, s.cout, s.k, s.stride, self.act,
                                            self.alpha, st), "adk_voc_convtr")
        else:
            native.check(lib.adk_voc_conv(_ptr(x), _ptr(self.wf), _ptr(bias), _ptr(res), _ptr(y), b, s.cin, t, s.cout, s.k, s.dilation,
                                          s.groups, self.act, self.alpha, self.impl, st), "adk_voc_conv")
        return y

    def grad_input(self, dy, x, wg, dres=None):
        """dy of the output's shape, x the saved input [+ dres of x's shape] -> dx."""
        s, lib = self.spec, native.lib()
        dx = torch.empty_like(x)
        b, _, t = x.shape
        st = native.current_stream(dy.device)
        xa = x if self.act != ACT_NONE else None
        if self.transposed:
            native.check(lib.adk_voc_convtr_grad(_ptr(dy), _ptr(xa), _ptr(wg), _ptr(dx), b, s.cin, t, s.cout, s.k, s.stride,
                                                 self.act, self.alpha, st), "adk_voc_convtr_grad")
        else:
            native.check(lib.adk_voc_conv_grad(_ptr(dy), _ptr(xa), _ptr(wg), _ptr(dres), _ptr(dx), b, s.cin, t, s.cout, s.k,
                                               s.dilation, s.groups, self.act, self.alpha, st), "adk_voc_conv_grad")
        return dx

    def grad_weight(self, dy, x, workspace, want_bias):
        """dy of the output's shape, x the saved input -> (dW in the reference's layout, db or None)."""
        s, lib = self.spec, native.lib()
        b, _, t = x.shape
        st = native.current_stream(dy.device)
        db = torch.empty(s.cout, dtype=torch.float32, device=dy.device) if want_bias else None
        dw = torch.empty(*s.wshape, dtype=torch.float32, device=dy.device)
        if self.transposed:
            n_bytes, _ = convtr_wgrad_plan(b, s.cin, t, s.cout, s.k, s.stride)
            ws = workspace.get(n_bytes, dy.device)
            native.check(lib.adk_voc_convtr_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), b, s.cin, t, s.cout, s.k, s.stride,
                                                  self.act, self.alpha, st), "adk_voc_convtr_wgrad")
        else:
            n_bytes, _ = conv_wgrad_plan(b, s.cin, t, s.cout, s.k, s.dilation, s.groups)
            ws = workspace.get(n_bytes, dy.device)
            native.check(lib.adk_voc_conv_wgrad(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), b, s.cin, t, s.cout, s.k, s.dilation,
                                                s.groups, self.act, self.alpha, st), "adk_voc_conv_wgrad")
        return dw, db


class _ConvFn(torch.autograd.Function):
    """One conv or transposed conv (with its input activation): backward to its input, its weight and its bias."""

    @staticmethod
    def forward(ctx, x, w, b, layer, workspace):
        ctx.layer, ctx.workspace, ctx.wg = layer, workspace, layer.wg
        ctx.save_for_backward(x)
        return layer.forward(x, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dy = _upstream(dy)
        dx = ctx.layer.grad_input(dy, x, ctx.wg) if need_x else None
        dw = db = None
        if need_w or need_b:
            dw, db = ctx.layer.grad_weight(dy, x, ctx.workspace, need_b)
        return dx, (dw if need_w else None), db, None, None


class _ResUnitFn(torch.autograd.Function):
    """One residual unit, x + convs2(a(convs1(a(x)))), or x + convs1(a(x)) when conv2 is None: the skip is the last conv's
    epilogue going forward and the first conv's going back."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, conv1, conv2, workspace):
        ctx.convs, ctx.workspace = (conv1, conv2), workspace
        ctx.wg = (conv1.wg, conv2.wg if conv2 is not None else None)
        if conv2 is None:
            ctx.save_for_backward(x)
            return conv1.forward(x, b1, res=x)
        h = conv1.forward(x, b1)
        ctx.save_for_backward(x, h)
        return conv2.forward(h, b2, res=x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        conv1, conv2 = ctx.convs
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:5]
        dy = _upstream(dy)
        dx = dw1 = db1 = dw2 = db2 = None
        if conv2 is None:
            (x,) = ctx.saved_tensors
            dh = dy
        else:
            x, h = ctx.saved_tensors
            if need_w2 or need_b2:
                dw2, db2 = conv2.grad_weight(dy, h, ctx.workspace, need_b2)
            dh = conv2.grad_input(dy, h, ctx.wg[1]) if (need_x or need_w1 or need_b1) else None
        if need_w1 or need_b1:
            dw1, db1 = conv1.grad_weight(dh, x, ctx.workspace, need_b1)
        if need_x:
            dx = conv1.grad_input(dh, x, ctx.wg[0], dres=dy)
        return dx, (dw1 if need_w1 else None), db1, (dw2 if need_w2 else None), db2, None, None, None


class TrainableVocoder(torch.nn.Module):
    """``models/vocoder/HiFiGAN.py``'s ``Generator`` as a trainable module: the constructor takes its parameters.
    ``forward(c)``: (B, in_channels, T) -> (B, out_channels, T * hop)."""

    _register = TrainableDecoder._register
    _param = TrainableDecoder._param

    def __init__(self, device=None, **generator_params):
        super().__init__()
        p = _merge(_HG_DEFAULTS, generator_params, "TrainableVocoder")
        assert p["kernel_size"] % 2 == 1, "Kernel size must be odd number."            # HiFiGAN.py:73-75
        assert len(p["upsample_scales"]) == len(p["upsample_kernel_sizes"])
        assert len(p["resblock_dilations"]) == len(p["resblock_kernel_sizes"])
        if p["nonlinear_activation"] != "LeakyReLU":
            raise NotImplementedError(f"nonlinear_activation {p['nonlinear_activation']!r}: TrainableVocoder implements LeakyReLU only")
        unknown = set(p["nonlinear_activation_params"] or {}) - {"negative_slope"}
        if unknown:
            raise NotImplementedError(f"nonlinear_activation_params {sorted(unknown)}: only LeakyReLU's negative_slope is implemented")
        for s, k in zip(p["upsample_scales"], p["upsample_kernel_sizes"]):
            if k != 2 * s:
                raise NotImplementedError(f"upsample kernel {k} with scale {s}: the transposed-conv kernels are written for kernel = 2 * scale")
        if min(p["in_channels"], p["out_channels"], p["channels"] >> len(p["upsample_scales"]), p["groups"], *p["upsample_scales"],
               *p["resblock_kernel_sizes"]) < 1:
            raise ValueError("in_channels, out_channels, channels / 2^stages, groups, upsample_scales and kernel sizes must be positive")
        self.params = p
        self.slope = float((p["nonlinear_activation_params"] or {}).get("negative_slope", OUTPUT_SLOPE))
        self.in_channels, self.out_channels = int(p["in_channels"]), int(p["out_channels"])
        self.hop = arch.hop_length(p)
        self.norm = p["stats"] is not None
        self.multigroup = arch.hifigan_is_multigroup(p)
        self.groups = int(p["groups"])
        self.additional = bool(p["use_additional_convs"])
        self._specs = arch.hifigan_convs(p)
        self._index = {s.name: i for i, s in enumerate(self._specs)}

        def act_of(s):                  # the activation the reference applies in front of each conv
            if s.name == "input_conv" or s.name.endswith(".conv_out"):
                return ACT_NONE, 0.0
            return (ACT_LEAKY, OUTPUT_SLOPE) if s.name == "output_conv" else (ACT_LEAKY, self.slope)

        self._layers = [_Layer(s, *act_of(s)) for s in self._specs]
        self._workspace = _Workspace()
        for s in self._specs:
            v = torch.empty(*s.wshape, dtype=torch.float32).normal_(0.0, 0.01)         # Generator.reset_parameters
            if s.wn:
                self._register(s.wkey("weight_g"), torch.linalg.vector_norm(v, 2, dim=(1, 2), keepdim=True))   # weight_norm: g = ||v||
                self._register(s.wkey("weight_v"), v)
            else:
                self._register(s.wkey("weight"), v)
            if s.bias:
                bound = 1.0 / math.sqrt(v.shape[1] * v.shape[2])                   # torch's fan-in: dim 1 x the kernel, both kinds
                self._register(s.wkey("bias"), torch.empty(s.cout, dtype=torch.float32).uniform_(-bound, bound))
        if self.norm:
            self.register_buffer("mean", torch.zeros(self.in_channels, dtype=torch.float32))
            self.register_buffer("scale", torch.ones(self.in_channels, dtype=torch.float32))
        if device is not None:
            self.to(native.require_gpu(device))

    @classmethod
    def from_generator(cls, gen, device=None):
        """A ``HiFiGANStreamGenerator`` as a trainable module with copies of its loaded weights; the generator is only read."""
        if gen._sd is None:
            raise RuntimeError("from_generator: the generator has no weights loaded (call load_state_dict first)")
        voc = cls(**gen.params)
        voc.load_state_dict(gen._sd)
        dev = device if device is not None else gen._device
        return voc.to(native.require_gpu(dev)) if dev is not None else voc

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The vocoder's checkpoint dict; the streaming ``*.pad_buffer`` entries are ignored."""
        own = {k: v for k, v in state_dict.items() if not k.endswith(".pad_buffer")}
        return super().load_state_dict(own, strict=strict, **kwargs)

    # ---- the structure: what forward and saved_floats both walk ----
    def _units(self, prefix, n):
        """The residual units of one HiFiGANResidualBlock: [(convs1.j index, convs2.j index or None)]."""
        ix = self._index
        return [(ix[f"{prefix}.convs1.{j}"], ix[f"{prefix}.convs2.{j}"] if self.additional else None) for j in range(n)]

    def _stage(self, i):
        """(upsample index, [chains of units], conv_out index or None) of stage i."""
        p, ix = self.params, self._index
        if self.multigroup:
            return ix[f"upsamples.{i}"], [self._units(f"blocks.{i}", len(p["resblock_dilations"][0]))], ix[f"blocks.{i}.conv_out"]
        chains = [self._units(f"blocks.{i}.blocks.{b}", len(d)) for b, d in enumerate(p["resblock_dilations"])]
        return ix[f"upsamples.{i}"], chains, None

    def saved_floats(self, batch, frames):
        """Floats a differentiable pass keeps until backward for a (batch, in_channels, frames) input: the pre-activation input of
        every conv (one tensor where several convs read the same one: the MRF's three chains start from the upsampler's output)
        and the output, which tanh's backward reads."""
        S, t = self._specs, frames
        n = batch * S[0].cin * t
        for i in range(len(self.params["upsample_scales"])):
            up, chains, out = self._stage(i)
            n += batch * S[up].cin * t
            t *= S[up].stride
            c = S[chains[0][0][0]].cin
            per_unit = 2 if self.additional else 1
            units = sum(len(ch) for ch in chains)
            # the first unit of every chain reads one shared tensor; every later conv reads a tensor of its own
            n += batch * c * t * (1 + units * per_unit - len(chains))
            if out is not None:
                n += batch * S[out].cin * t
        n += batch * S[-1].cin * t
        return n + batch * self.out_channels * t

    def _weights(self, grad):
        """Per conv (w, bias): w the composed weight with its graph when grad is asked for, else None; the layer's packings are
        brought up to date with the parameters."""
        out = []
        for s, layer in zip(self._specs, self._layers):
            src = (self._param(s.wkey("weight_g")), self._param(s.wkey("weight_v"))) if s.wn else (self._param(s.wkey("weight")),)
            key = tuple((q._version, q.data_ptr(), q.device) for q in src)
            w = None
            if grad or layer.stale(key):
                w = weight_norm(*src) if s.wn else src[0]
            if layer.stale(key):
                layer.repack(key, w)
            out.append((w if grad else None, self._param(s.wkey("bias")) if s.bias else None))
        return out

    def forward(self, c):
        if not isinstance(c, torch.Tensor) or c.dim() != 3 or c.shape[1] != self.in_channels:
            raise ValueError(f"expected a (B, {self.in_channels}, T) input, got {tuple(getattr(c, 'shape', ()))}")
        if c.shape[0] == 0 or c.shape[2] == 0:
            raise ValueError(f"empty input {tuple(c.shape)}")
        params = list(self.parameters())
        dev = params[0].device
        if any(q.dtype != torch.float32 or q.device != dev for q in params):
            raise TypeError("TrainableVocoder computes in float32 with every parameter on one device")
        native.require_gpu(dev)
        c = _settled(c)
        grad = torch.is_grad_enabled() and (c.requires_grad or any(q.requires_grad for q in params))
        L, ws = self._layers, self._workspace
        with torch.set_grad_enabled(grad):
            P = self._weights(grad)
            x = c.to(device=dev, dtype=torch.float32)
            if self.norm:
                x = (x - self.mean[None, :, None]) / self.scale[None, :, None]
            x = x.contiguous()
            if grad:
                conv = lambda h, i: _ConvFn.apply(h, P[i][0], P[i][1], L[i], ws)                                  # noqa: E731
                unit = lambda h, i, j: _ResUnitFn.apply(h, P[i][0], P[i][1], P[j][0] if j is not None else None,  # noqa: E731
                                                        P[j][1] if j is not None else None, L[i], L[j] if j is not None else None, ws)
            else:
                conv = lambda h, i: L[i].forward(h, P[i][1])                                                      # noqa: E731
                unit = lambda h, i, j: (L[i].forward(h, P[i][1], res=h) if j is None else                         # noqa: E731
                                        L[j].forward(L[i].forward(h, P[i][1]), P[j][1], res=h))
            h = conv(x, 0)
            for i in range(len(self.params["upsample_scales"])):
                up, chains, out = self._stage(i)
                h = conv(h, up)
                if self.multigroup:
                    h = h.repeat(1, self.groups, 1)
                    for a, b in chains[0]:
                        h = unit(h, a, b)
                    h = conv(h, out)
                else:
                    cs = 0.0                                # MultiReceptiveField.forward's sum, in its order
                    for chain in chains:
                        x = h
                        for a, b in chain:
                            x = unit(x, a, b)
                        cs = cs + x
                    h = (cs / len(chains)).contiguous()
            return torch.tanh(conv(h, len(L) - 1))
