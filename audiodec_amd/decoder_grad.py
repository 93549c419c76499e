"""The symmetric decoder as a frozen, differentiable function of its input, and the quantizer's straight-through step
(adk_dec_conv, adk_dec_convtr, their ``_grad`` calls and adk_rvq_st_grad: csrc/dec_grad.hip).

The reference's denoising flow (``trainer/denoise.py``) freezes the quantizer and the decoder and trains the encoder alone on
the VQ loss plus the metric loss of ``decoder(quantizer(encoder(x_noisy)))`` against the clean signal.  With the device metric
losses' ``differentiable=True`` a gradient reaches ``y_hat``; ``FrozenDecoder`` carries it to ``zq`` and ``quantize_st`` to ``z``,
where a torch encoder's own autograd takes over.

``FrozenDecoder`` mirrors ``models/autoencoder/modules/decoder.py:79-138`` (``Decoder``, 'causal' mode, ELU) with the reference's
constructor arguments and state-dict keys.  Its forward is the non-streaming ``Decoder.forward`` on (B, C, T) tensors: one HIP
call per conv, exact f32, every layer's output written to memory.  With grad enabled and an input that requires grad, conv1,
conv2, every transposed conv and every residual unit (its two convs and its skip) is a ``torch.autograd.Function`` whose backward
is the matching ``_grad`` call; what is saved is the pre-activation input of every conv that has an input activation (the
residual units' inputs and inner activations).  The weights are constants: nothing here is a parameter and no weight gradient
exists.  The backward is once-differentiable and, like the forward, bitwise reproducible.  Otherwise the same kernels run with no
graph and nothing saved, so the output is bitwise the same.

The streaming generators, their programs, rings and guard are not used and not touched.
"""
import torch

from . import arch, native, program
from .loss_common import _ptr, _settled

ACT_NONE, ACT_ELU = 0, 1
IMPL_DIRECT, IMPL_GEMM = 1, 2
DIRECT_MAX_COUT = 2                 # conv2 (C_out = 1 or 2) runs on the direct kernel: a 32-row GEMM tile would be 31/32 empty


# ---- weight packings (host, once per load) ---------------------------------------------------------------------------------
def pack_conv(w):
    """Conv1d weight (C_out, C_in, k) -> the forward GEMM's [kk = ci*k + j][co]."""
    co, ci, k = w.shape
    return w.reshape(co, ci * k).t().contiguous()


def pack_conv_grad(w):
    """Conv1d weight (C_out, C_in, k) -> the backward-data GEMM's [kk = co*k + j][ci]."""
    co, ci, k = w.shape
    return w.permute(0, 2, 1).reshape(co * k, ci).contiguous()


def pack_convtr(w, stride):
    """ConvTranspose1d weight (C_in, C_out, 2s) -> the polyphase forward GEMMs' [r][kk = 2*ci + tap][co]: tap 0 is W[ci][co][r]
    (frame i), tap 1 is W[ci][co][s + r] (frame i - 1)."""
    ci, co, k = w.shape
    if k != 2 * stride:
        raise ValueError(f"transposed conv: kernel {k} is not 2 * stride = {2 * stride}")
    return w.reshape(ci, co, 2, stride).permute(3, 0, 2, 1).reshape(stride, 2 * ci, co).contiguous()


def pack_convtr_grad(w, stride):
    """ConvTranspose1d weight (C_in, C_out, 2s) -> the backward-data GEMM's [kk = co*2s + q][ci]."""
    ci, co, k = w.shape
    if k != 2 * stride:
        raise ValueError(f"transposed conv: kernel {k} is not 2 * stride = {2 * stride}")
    return w.permute(1, 2, 0).reshape(co * k, ci).contiguous()


# ---- one layer's device weights and its two native calls -------------------------------------------------------------------
class _Layer:
    """spec: arch.ConvSpec; act/alpha: the INPUT activation the reference applies in front of this conv."""

    def __init__(self, spec, w, b, act, alpha, dev):
        self.spec, self.act, self.alpha = spec, act, float(alpha)
        self.bias = b.float().contiguous().to(dev) if b is not None else None
        if spec.kind == "convT":
            self.impl = IMPL_GEMM
            self.w = pack_convtr(w, spec.stride).to(dev)
            self.w_grad = pack_convtr_grad(w, spec.stride).to(dev)
        else:
            self.impl = IMPL_DIRECT if spec.cout <= DIRECT_MAX_COUT else IMPL_GEMM
            self.w = (w.contiguous() if self.impl == IMPL_DIRECT else pack_conv(w)).to(dev)
            self.w_grad = pack_conv_grad(w).to(dev)

    def out_shape(self, x_shape):
        b, c, t = x_shape
        if c != self.spec.cin:
            raise ValueError(f"{self.spec.name}: input has {c} channels, the layer takes {self.spec.cin}")
        return b, self.spec.cout, t * self.spec.stride

    def __call__(self, x, res=None):
        """x (B, C_in, T) contiguous float32 [+ res of the output's shape] -> (B, C_out, T * stride)."""
        s, lib = self.spec, native.lib()
        y = torch.empty(*self.out_shape(x.shape), dtype=torch.float32, device=x.device)
        b, _, t = x.shape
        st = native.current_stream(x.device)
        if s.kind == "convT":
            native.check(lib.adk_dec_convtr(_ptr(x), _ptr(self.w), _ptr(self.bias), _ptr(y), b, s.cin, t, s.cout, s.k, s.stride,
                                            self.act, self.alpha, st), "adk_dec_convtr")
        else:
            native.check(lib.adk_dec_conv(_ptr(x), _ptr(self.w), _ptr(self.bias), _ptr(res), _ptr(y), b, s.cin, t, s.cout, s.k,
                                          s.dilation, self.act, self.alpha, self.impl, st), "adk_dec_conv")
        return y

    def grad(self, dy, x, x_shape, dres=None):
        """dy of the output's shape, x the saved input (None without an input activation) [+ dres of x's shape] -> dx."""
        s, lib = self.spec, native.lib()
        dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
        b, _, t = x_shape
        st = native.current_stream(dy.device)
        if s.kind == "convT":
            native.check(lib.adk_dec_convtr_grad(_ptr(dy), _ptr(x), _ptr(self.w_grad), _ptr(dx), b, s.cin, t, s.cout, s.k,
                                                 s.stride, self.act, self.alpha, st), "adk_dec_convtr_grad")
        else:
            native.check(lib.adk_dec_conv_grad(_ptr(dy), _ptr(x), _ptr(self.w_grad), _ptr(dres), _ptr(dx), b, s.cin, t, s.cout,
                                               s.k, s.dilation, self.act, self.alpha, st), "adk_dec_conv_grad")
        return dx


def _upstream(dy):
    return dy.to(torch.float32).contiguous()


class _ConvFn(torch.autograd.Function):
    """One conv or transposed conv (with its input activation) with a backward to its input."""

    @staticmethod
    def forward(ctx, x, layer):
        ctx.layer, ctx.x_shape = layer, tuple(x.shape)
        if layer.act != ACT_NONE:
            ctx.save_for_backward(x)
        return layer(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x = ctx.saved_tensors[0] if ctx.saved_tensors else None
        return ctx.layer.grad(_upstream(dy), x, ctx.x_shape), None


class _ResUnitFn(torch.autograd.Function):
    """One residual unit, x + conv2(a(conv1(a(x)))): the skip is conv2's epilogue going forward and conv1's going back."""

    @staticmethod
    def forward(ctx, x, conv1, conv2):
        ctx.convs, ctx.x_shape = (conv1, conv2), tuple(x.shape)
        h = conv1(x)
        ctx.save_for_backward(x, h)
        return conv2(h, res=x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        conv1, conv2 = ctx.convs
        x, h = ctx.saved_tensors
        dy = _upstream(dy)
        dh = conv2.grad(dy, h, tuple(h.shape))
        return conv1.grad(dh, x, ctx.x_shape, dres=dy), None, None


def _res_unit(x, conv1, conv2):
    return conv2(conv1(x), res=x)


# ---- the decoder -----------------------------------------------------------------------------------------------------------
class FrozenDecoder:
    """``Decoder(code_dim, output_channels, decode_channels, ...)`` of the reference with constant weights and a backward to its
    input.  ``forward(zq)``: (B, code_dim, T) -> (B, output_channels, T * hop)."""

    def __init__(self, code_dim, output_channels, decode_channels, channel_ratios=(16, 8, 4, 2), strides=(5, 5, 4, 3), kernel_size=7,
                 bias=True, mode="causal", nonlinear_activation="ELU", nonlinear_activation_params={}, device=None,
                 use_weight_norm=False, codec="audiodec"):
        if codec != "audiodec":
            raise NotImplementedError(f"codec {codec!r}: FrozenDecoder implements Decoder only, not ActivateDecoder")
        if mode != "causal":
            raise NotImplementedError(f"mode {mode!r}: FrozenDecoder implements the causal decoder only")
        if nonlinear_activation != "ELU":
            raise NotImplementedError(f"nonlinear_activation {nonlinear_activation!r}: FrozenDecoder implements ELU only")
        unknown = set(nonlinear_activation_params or {}) - {"alpha"}
        if unknown:
            raise NotImplementedError(f"nonlinear_activation_params {sorted(unknown)}: only ELU's alpha is implemented")
        if len(channel_ratios) != len(strides):
            raise ValueError("channel_ratios and strides must have the same length")
        if kernel_size != 7:
            raise NotImplementedError("kernel_size: the reference's residual units and this class are written for 7")
        if min(code_dim, output_channels, decode_channels, *channel_ratios, *strides) < 1:
            raise ValueError("code_dim, output_channels, decode_channels, channel_ratios and strides must be positive")
        self.alpha = float((nonlinear_activation_params or {}).get("alpha", 1.0))
        self.params = dict(code_dim=int(code_dim), output_channels=int(output_channels), decode_channels=int(decode_channels),
                           dec_ratios=tuple(channel_ratios), dec_strides=tuple(strides), bias=bool(bias),
                           use_weight_norm=bool(use_weight_norm), codec="audiodec")
        self.code_dim, self.output_channels = int(code_dim), int(output_channels)
        self.hop = 1
        for s in strides:
            self.hop *= int(s)
        self._specs = arch.autoencoder_decoder_convs(self.params)
        self._host = self._layers = None
        self._dev = torch.device(device) if device is not None else None
        if self._dev is not None:
            native.require_gpu(self._dev)

    @classmethod
    def from_generator(cls, gen, device=None):
        """The decoder of an ``AutoEncoderStreamGenerator`` with its loaded weights; the generator is only read."""
        p = gen.params
        if gen._sd is None:
            raise RuntimeError("from_generator: the generator has no weights loaded (call load_state_dict first)")
        dec = cls(p["code_dim"], p["output_channels"], p["decode_channels"], p["dec_ratios"], p["dec_strides"], 7, p["bias"],
                  p["mode"], p["nonlinear_activation"], p["nonlinear_activation_params"],
                  device=device if device is not None else gen._device, use_weight_norm=p["use_weight_norm"], codec=p["codec"])
        return dec.load_state_dict(gen._sd)

    def state_dict_keys(self):
        """The generator's keys of the decoder's weights (``decoder.*``; pad buffers are not state of the non-streaming forward)."""
        keys = []
        for s in self._specs:
            keys += [s.wkey("weight_g"), s.wkey("weight_v")] if s.wn else [s.wkey("weight")]
            if s.bias:
                keys.append(s.wkey("bias"))
        return keys

    def load_state_dict(self, state_dict):
        """The generator's keys (``decoder.*``; everything else is ignored) or the decoder's own (no prefix).  Weight norm is folded
        as the generators fold it (``torch._weight_norm(v, g, 0)``)."""
        sd = dict(state_dict)
        if not any(k.startswith("decoder.") for k in sd):
            sd = {f"decoder.{k}": v for k, v in sd.items()}
        missing = [k for k in self.state_dict_keys() if k not in sd]
        if missing:
            raise RuntimeError(f"Error(s) in loading state_dict for FrozenDecoder: missing keys {missing[:8]}{'...' if len(missing) > 8 else ''}")
        host = []
        for s in self._specs:
            w = program.effective_weight(sd, s).detach().cpu().contiguous()
            if tuple(w.shape) != tuple(s.wshape):
                raise RuntimeError(f"size mismatch for {s.wkey()}: {tuple(w.shape)} in the state dict, {tuple(s.wshape)} configured")
            host.append((s, w, sd[s.wkey("bias")].detach().float().cpu() if s.bias else None))
        self._host, self._layers = host, None
        if self._dev is not None:
            self.to(self._dev)
        return self

    def to(self, device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        native.require_gpu(dev)
        if self._dev != dev or self._layers is None:
            self._dev = dev
            if self._host is not None:
                # the input activation of each conv: the residual units' two convs have one, nothing else (decoder.py, residual_unit.py:45-48)
                self._layers = [_Layer(s, w, b, ACT_ELU if ".res_units." in s.name else ACT_NONE, self.alpha, dev)
                                for s, w, b in self._host]
        return self

    @property
    def device(self):
        return self._dev

    def weights(self):
        """Every device tensor this decoder computes with (none requires grad)."""
        return [t for L in self._layers or [] for t in (L.w, L.w_grad, L.bias) if t is not None]

    def saved_floats(self, batch, frames):
        """Floats a differentiable pass keeps until backward for a (batch, code_dim, frames) input: two tensors per residual unit."""
        n, t = 0, frames
        for s in self._specs:
            t *= s.stride if s.kind == "convT" else 1
            if ".res_units." in s.name:
                n += batch * s.cin * t
        return n

    def forward(self, zq):
        if not isinstance(zq, torch.Tensor) or zq.dim() != 3 or zq.shape[1] != self.code_dim:
            raise ValueError(f"expected a (B, {self.code_dim}, T) input, got {tuple(getattr(zq, 'shape', ()))}")
        if self._host is None:
            raise RuntimeError("FrozenDecoder: no weights loaded (call load_state_dict first)")
        zq = _settled(zq)
        if self._dev is None or self._layers is None:
            self.to(self._dev if self._dev is not None else
                    (zq.device if zq.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())))
        grad = torch.is_grad_enabled() and zq.requires_grad
        x = zq.to(device=self._dev, dtype=torch.float32).contiguous()
        if x.shape[0] == 0 or x.shape[2] == 0:
            raise ValueError(f"empty input {tuple(zq.shape)}")
        L = self._layers
        conv = (lambda h, layer: _ConvFn.apply(h, layer)) if grad else (lambda h, layer: layer(h))
        unit = (lambda h, c1, c2: _ResUnitFn.apply(h, c1, c2)) if grad else _res_unit
        x = conv(x, L[0])
        i = 1
        while i < len(L) - 1:
            x = conv(x, L[i])                                  # the block's transposed conv, then its residual units
            i += 1
            while i < len(L) - 1 and L[i].spec.kind != "convT":
                x = unit(x, L[i], L[i + 1])
                i += 2
        return conv(x, L[-1])

    __call__ = forward


# ---- the quantizer's straight-through step ---------------------------------------------------------------------------------
class _QuantizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gen):
        zc = z.detach().to(device=gen._dev(), dtype=torch.float32).contiguous()
        flat, idx0 = _quantizer_forward_stats(gen, zc)
        B, D, T = zc.shape
        n = B * T * D
        ctx.gen, ctx.shape, ctx.z_like = gen, (B, D, T), (z.device, z.dtype)
        ctx.save_for_backward(zc, idx0)
        zq, vq, ppl = flat[:n].view(B, T, D).transpose(2, 1), flat[n:n + gen.n_q], flat[n + gen.n_q:]
        ctx.mark_non_differentiable(ppl)
        return zq, vq, ppl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dzq, dvq, _dppl):
        z, idx0 = ctx.saved_tensors
        B, D, T = ctx.shape
        gen = ctx.gen
        dzq = _upstream(dzq) if dzq is not None else None
        dvq = _upstream(dvq) if dvq is not None else None
        dz = torch.empty_like(z)
        native.check(native.lib().adk_rvq_st_grad(_ptr(dzq), _ptr(dvq), _ptr(z), _ptr(gen._codebook), _ptr(idx0), _ptr(dz), B, D, T,
                                                  gen.size, native.current_stream(z.device)), "adk_rvq_st_grad")
        return dz.to(device=ctx.z_like[0], dtype=ctx.z_like[1]), None


def _quantizer_forward_stats(gen, z):
    """What ``gen._quantizer_forward_stats`` computes, with the same calls in the same order (so the same values, bit for bit), and
    stage 0's indices, which the backward looks its codes up with.  (That method drops the indices, and stream_generator.py is
    part of the digest the committed profiles are keyed on, so it is restated here rather than changed there;
    tests/test_gpu_decoder_grad.py holds the two together bit for bit.)"""
    from . import codebook_usage
    dev = gen._dev()
    embed, enorm = gen._quantizer()
    if gen._codebook is None:
        gen.initial()
    B, D, T = z.shape
    n = B * T * D
    zt = z.transpose(2, 1).contiguous()
    idx = torch.empty(gen.n_q, B * T, dtype=torch.int64, device=dev)
    out = torch.empty(n + 2 * gen.n_q, dtype=torch.float32, device=dev)
    native.check(native.lib().adk_rvq_encode(_ptr(zt), _ptr(embed), _ptr(enorm), _ptr(idx), _ptr(out), B * T, gen.n_q, gen.dim,
                                             gen.size, native.current_stream(dev)), "adk_rvq_encode")
    acc = codebook_usage.accumulator(gen.n_q, gen.size, dev)
    codebook_usage.fold(acc, zt.view(B * T, D), gen._codebook, idx, gen.n_q, gen.dim, gen.size, out[n:n + gen.n_q], out[n + gen.n_q:])
    return out, idx[0].contiguous()


def quantize_st(gen, z):
    """``Quantizer.forward`` in eval mode with its straight-through gradient: z (B, code_dim, T) -> (zq, vqloss, perplexity), the
    values of ``gen.quantizer_forward(z, return_stats=True)``.  When z requires grad (and grad is enabled), zq and vqloss carry a
    node whose backward is adk_rvq_st_grad: stage 0 passes zq's gradient straight through and vqloss[0] adds
    2 (z - q0) / (rows * dim); stages >= 1 see a residual that is a constant to autograd (layers/vq_module.py:119-134).  The
    codebooks are constants.  The call settles the generator's call log first and is not logged itself, as the ``ema=`` path."""
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[1] != gen.dim:
        raise ValueError(f"expected a (B, {gen.dim}, T) latent, got {tuple(getattr(z, 'shape', ()))}")
    if z.shape[0] == 0 or z.shape[2] == 0:
        raise ValueError(f"empty latent {tuple(z.shape)}")
    gen.settle()
    z = _settled(z)
    if torch.is_grad_enabled() and z.requires_grad:
        return _QuantizeFn.apply(z, gen)
    flat, _ = _quantizer_forward_stats(gen, z.detach().to(device=gen._dev(), dtype=torch.float32).contiguous())
    B, D, T = z.shape
    n = B * T * D
    return flat[:n].view(B, T, D).transpose(2, 1), flat[n:n + gen.n_q], flat[n + gen.n_q:]
