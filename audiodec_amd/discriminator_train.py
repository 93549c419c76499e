"""The HiFi-GAN discriminator as a trainable module on the HIP path (adk_disc_conv_wgrad: csrc/disc_wgrad.hip; adk_disc_conv,
adk_disc_conv_grad, adk_disc_prep and the loss calls: csrc/disc.hip).

The reference's GAN flow updates the discriminator on its own step (``trainer/trainerGAN.py:256-294``,
``trainer/autoencoder.py:117-126``): ``D(x)``, ``D(y_.detach())``, ``real_loss + fake_loss``, ``backward()``, ``clip_grad_norm_``,
``optimizer.step()``.  ``discriminator.Discriminator`` computes the forward and the backward to its input with constant weights;
this module adds the gradient to the weights and owns them as parameters.

``TrainableDiscriminator`` mirrors ``models/vocoder/HiFiGAN.py:308-395`` ``Discriminator`` as one ``torch.nn.Module`` whose
parameters carry the reference's state-dict keys, exactly ``discriminator.Discriminator(...).state_dict_keys()``: ``weight`` /
``bias`` for the scale discriminators' Conv1d layers, ``weight_g`` / ``weight_v`` / ``bias`` for the period discriminators'
weight-normed (k, 1) Conv2d layers (``weight`` without weight norm).  Its forward is ``discriminator.Discriminator``'s: one
adk_disc_conv call per layer on weights packed from the composed weight (``conv_impl`` chooses the kernel), reflect padding and
pooling through adk_disc_prep; under ``no_grad`` the feature maps are bitwise those of ``discriminator.Discriminator`` loaded with
this module's ``state_dict()``.  With grad enabled and anything asking for a gradient every conv is a once-differentiable
``torch.autograd.Function`` whose backward returns dx (adk_disc_conv_grad), dW and db (adk_disc_conv_wgrad) and skips what
``needs_input_grad`` does not ask for: no first-layer dx when the waveform does not require grad (the discriminator step), no
weight gradient for a layer whose parameters are frozen (the generator step, where the module behaves as
``discriminator.Discriminator(differentiable=True)``).  What is kept until backward is the feature pyramid: a layer's input is
the previous layer's output.  The weight-norm composition ``w = v g / ||v||`` stays torch (``torch._weight_norm``, the call
``discriminator.effective_weight`` folds a checkpoint with) and is differentiated by autograd.  Forward and gradients are bitwise
reproducible.

The kernels read re-packed weights; the packings are rebuilt on the device, under ``no_grad``, when a parameter's version
counter, storage or device has changed (an optimizer step, ``load_state_dict``), not on every call.

``DiscriminatorAdversarialLoss`` here is ``discriminator.DiscriminatorAdversarialLoss`` with a backward (adk_disc_loss_grad).
"""
import ctypes as C
import math

import torch

from . import discriminator as D
from . import lazy_guard, native
from .decoder_grad import _upstream
from .decoder_train import TrainableDecoder
from .discriminator import (ACT_LEAKY, ACT_NONE, IMPL_DIRECT, MPD_DISC_DEFAULTS, MSD_DISC_DEFAULTS, POOL_DEFAULTS, PREP_AVGPOOL,
                            PREP_REFLECT, conv_impl, conv_out_len, pack_grad_weights, pool_out_len, reflect_pad_len)
from .encoder_grad import _Workspace
from .loss_common import _ptr, _settled


def conv_wgrad_plan(n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad):
    """(workspace bytes, slices) of adk_disc_conv_wgrad for a shape; host only."""
    ws, s = C.c_int64(0), C.c_int32(0)
    native.check(native.lib().adk_disc_conv_wgrad_plan(n_items, c_in, h_in, period, c_out, groups, kernel, stride, pad,
                                                       C.byref(ws), C.byref(s)), "adk_disc_conv_wgrad_plan")
    return int(ws.value), int(s.value)


def weight_norm(g, v):
    """torch.nn.utils.weight_norm's composition over dim 0, w = v g / ||v|| with the norm per slice v[i]: the call the
    reference's pre-hook makes and ``discriminator.effective_weight`` folds a checkpoint with, so that a state dict taken from
    this module gives ``discriminator.Discriminator`` the weights this module computes with."""
    return torch._weight_norm(v, g, 0)


class _Layer:
    """One conv of the discriminator: its description, its kernel, and the packed forms of its composed weight."""

    def __init__(self, layer):
        self.layer, self.impl = layer, conv_impl(layer)
        self.act = ACT_LEAKY if layer.act_slope is not None else ACT_NONE
        self.slope = float(layer.act_slope or 0.0)
        self.geometry = (layer.cout, layer.groups, layer.kernel, layer.stride, layer.pad)
        self._key = None
        self.wf = self.wg = None        # forward packing, backward-data packing

    def stale(self, key):
        return key != self._key

    def repack(self, key, w):
        """The packings of the composed weight w (the reference's layout), kept under the parameters' key."""
        L = self.layer
        with torch.no_grad():
            wd = L.fold(w.detach()).contiguous()
            if self.impl == IMPL_DIRECT:
                self.wf = self.wg = wd.clone()
            else:
                self.wf = wd.reshape(L.groups, L.cout // L.groups, -1).permute(0, 2, 1).contiguous()   # [g][cin_g * k][cout_g]
                self.wg = pack_grad_weights(wd, L)
        self._key = key

    def out_shape(self, x_shape):
        L = self.layer
        n, _, h, p = x_shape
        ho = conv_out_len(h, L)
        if ho < 1:
            raise ValueError(f"{L.key}: input length {h} is shorter than the kernel {L.kernel} with padding {L.pad}")
        return n, L.cout, ho, p

    def forward(self, x, bias):
        """x (N, C_in, H, P) contiguous float32 -> (N, C_out, H', P)."""
        y = torch.empty(*self.out_shape(x.shape), dtype=torch.float32, device=x.device)
        native.check(native.lib().adk_disc_conv(_ptr(x), _ptr(self.wf), _ptr(bias), _ptr(y), *x.shape, *self.geometry, self.act,
                                                self.slope, self.impl, native.current_stream(x.device)), "adk_disc_conv")
        return y

    def grad_input(self, dy, y, x_shape, wg):
        """dy, y of the output's shape -> dx of x_shape."""
        dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
        ya = y if self.act != ACT_NONE else None
        native.check(native.lib().adk_disc_conv_grad(_ptr(dy), _ptr(ya), _ptr(wg), _ptr(dx), *x_shape, *self.geometry, self.act,
                                                     self.slope, self.impl, native.current_stream(dy.device)), "adk_disc_conv_grad")
        return dx

    def grad_weight(self, dy, y, x, workspace, want_bias):
        """dy, y of the output's shape, x the layer's input -> (dW (C_out, C_in/g, k), db or None)."""
        L = self.layer
        n_bytes, _ = conv_wgrad_plan(*x.shape, *self.geometry)
        ws = workspace.get(n_bytes, dy.device)
        dw = torch.empty(*L.weight_shape, dtype=torch.float32, device=dy.device)
        db = torch.empty(L.cout, dtype=torch.float32, device=dy.device) if want_bias else None
        ya = y if self.act != ACT_NONE else None
        native.check(native.lib().adk_disc_conv_wgrad(_ptr(dy), _ptr(ya), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), *x.shape,
                                                      *self.geometry, self.act, self.slope, native.current_stream(dy.device)),
                     "adk_disc_conv_wgrad")
        return dw, db


class _ConvFn(torch.autograd.Function):
    """One conv layer (with its activation): backward to its input, its weight and its bias.  x is the previous layer's output
    and y this layer's: what is saved is the feature pyramid."""

    @staticmethod
    def forward(ctx, x, w, b, layer, workspace):
        ctx.layer, ctx.workspace, ctx.wg = layer, workspace, layer.wg
        ctx.w_shape = tuple(w.shape) if w is not None else None
        y = layer.forward(x, b)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dy = _upstream(dy)
        dx = ctx.layer.grad_input(dy, y, tuple(x.shape), ctx.wg) if need_x else None
        dw = db = None
        if need_w or need_b:
            dw, db = ctx.layer.grad_weight(dy, y, x, ctx.workspace, need_b)
        return dx, (dw.reshape(ctx.w_shape) if need_w else None), db, None, None


class TrainableDiscriminator(torch.nn.Module):
    """``models/vocoder/HiFiGAN.py:308-395`` ``Discriminator`` as a trainable module: ``discriminator.Discriminator``'s arguments
    and defaults.  ``forward(x)``: (B, C, T), C != 1 read as (B*C, 1, T) -> the reference's list (one per sub-discriminator) of
    lists of per-layer feature maps."""

    _register = TrainableDecoder._register
    _param = TrainableDecoder._param

    def __init__(self, scales=3, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=POOL_DEFAULTS,
                 scale_discriminator_params=MSD_DISC_DEFAULTS, follow_official_norm=True, periods=[2, 3, 5, 7, 11],
                 period_discriminator_params=MPD_DISC_DEFAULTS, device=None):
        super().__init__()
        # the layer descriptions, the pooling and the checks of the arguments are discriminator.Discriminator's (no device: host only)
        desc = D.Discriminator(scales=scales, scale_downsample_pooling=scale_downsample_pooling,
                               scale_downsample_pooling_params=scale_downsample_pooling_params,
                               scale_discriminator_params=scale_discriminator_params, follow_official_norm=follow_official_norm,
                               periods=periods, period_discriminator_params=period_discriminator_params, differentiable=True)
        self._scale_layers, self._period_layers = desc.msd.discriminator_layers, desc.mpd.discriminator_layers
        self._pool, self._periods = desc.msd.pool, desc.mpd.periods
        self.discriminator_layers = desc.discriminator_layers
        self._descs = list(desc._layers)
        self._keys = desc.state_dict_keys()
        if any(L.norm == "spectral" for L in self._descs):
            raise NotImplementedError("use_spectral_norm=True: spectral-norm parameters (weight_orig / weight_u) are not implemented "
                                      "on the HIP discriminator")
        self._layers = {L.key: _Layer(L) for L in self._descs}
        self._workspace = _Workspace()
        # The reference's Discriminator has no reset_parameters of its own (HiFiGAN.py:308-395; modules/discriminator.py:27-449 call
        # none either, unlike Generator.reset_parameters at HiFiGAN.py:164-177): its convs keep torch's Conv1d / Conv2d
        # initialisation, and nn.utils.weight_norm (discriminator.py:140-148) then sets g = ||v||.
        for L in self._descs:
            shape = (*L.weight_shape, 1) if L.conv2d else L.weight_shape
            v = torch.empty(*shape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(v, a=math.sqrt(5))                       # torch's _ConvNd.reset_parameters
            if L.norm == "weight":
                self._register(f"{L.key}.weight_g", torch.linalg.vector_norm(v, 2, dim=tuple(range(1, v.dim())), keepdim=True))
                self._register(f"{L.key}.weight_v", v)
            else:
                self._register(f"{L.key}.weight", v)
            if L.bias:
                bound = 1.0 / math.sqrt(L.weight_shape[1] * L.weight_shape[2])      # torch's fan-in: dim 1 x the kernel
                self._register(f"{L.key}.bias", torch.empty(L.cout, dtype=torch.float32).uniform_(-bound, bound))
        if device is not None:
            self.to(native.require_gpu(device))

    @property
    def n_discriminators(self):
        return len(self.discriminator_layers)

    def state_dict_keys(self):
        return list(self._keys)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The reference's discriminator checkpoint dict (``checkpoint["model"]["discriminator"]``); spectral-norm keys raise."""
        for k in state_dict:
            if k.endswith(".weight_orig") or k.endswith(".weight_u"):
                raise NotImplementedError(f"{k}: spectral-norm parameters are not implemented on the HIP discriminator")
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    def _weights(self, grad):
        """Per layer key (w, bias): w the composed weight with its graph when one of its parameters asks for a gradient, else
        None; the layer's packings are brought up to date with the parameters."""
        out = {}
        for L in self._descs:
            layer = self._layers[L.key]
            wn = L.norm == "weight"
            src = (self._param(f"{L.key}.weight_g"), self._param(f"{L.key}.weight_v")) if wn else (self._param(f"{L.key}.weight"),)
            key = tuple((q._version, q.data_ptr(), q.device) for q in src)
            want = grad and any(q.requires_grad for q in src)
            w = None
            if want or layer.stale(key):
                w = weight_norm(*src) if wn else src[0]
            if layer.stale(key):
                layer.repack(key, w)
            out[L.key] = (w if want else None, self._param(f"{L.key}.bias") if L.bias else None)
        return out

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError(f"expected a (B, C, T) input, got shape {tuple(getattr(x, 'shape', ()))}")
        params = list(self.parameters())
        dev = params[0].device
        if any(q.dtype != torch.float32 or q.device != dev for q in params):
            raise TypeError("TrainableDiscriminator computes in float32 with every parameter on one device")
        native.require_gpu(dev)
        x = _settled(x)
        grad_x = torch.is_grad_enabled() and x.requires_grad
        grad = torch.is_grad_enabled() and (x.requires_grad or any(q.requires_grad for q in params))
        ws = self._workspace
        with torch.set_grad_enabled(grad):
            P = self._weights(grad)
            x = x.to(device=dev, dtype=torch.float32).contiguous()
            b, c, t = x.shape
            if c != 1:
                x = x.reshape(b * c, 1, t)                                             # HiFiGAN.py:390-392
                b, c = b * c, 1

            def conv(h, L):
                w, bias = P[L.key]
                layer = self._layers[L.key]
                return _ConvFn.apply(h, w, bias, layer, ws) if grad else layer.forward(h, bias)

            outs = []
            cur, n = x, t
            for d, layers in enumerate(self._scale_layers):                           # discriminator.py:444-447
                h, o = cur.reshape(b, c, n, 1), []
                for L in layers:
                    h = conv(h, L)
                    o.append(h.reshape(h.shape[0], h.shape[1], h.shape[2]))
                outs.append(o)
                if d + 1 < len(self._scale_layers):
                    k, s, p = self._pool
                    n2 = pool_out_len(n, k, s, p)
                    if n2 < 1:
                        raise ValueError(f"input length {t}: too short for {len(self._scale_layers)} scales")
                    cur = D._prep_op(cur, b * c, n, PREP_AVGPOOL, k, s, p, n_out=n2, grad=grad_x).reshape(b, c, n2)
                    n = n2
            for period, layers in zip(self._periods, self._period_layers):             # discriminator.py:121-136
                n_pad = reflect_pad_len(t, period)
                if n_pad >= t:
                    raise ValueError(f"input length {t}: reflect padding of {n_pad} for period {period} needs more than {n_pad} "
                                     "samples (F.pad raises for it too)")
                xp = D._prep_op(x, b * c, t, PREP_REFLECT, n_pad, n_out=t + n_pad, grad=grad_x) if n_pad else x
                h, o = xp.reshape(b, c, (t + n_pad) // period, period), []
                for l, L in enumerate(layers):
                    h = conv(h, L)
                    o.append(h if l + 1 < len(layers) else h.reshape(b, -1))          # torch.flatten(x, 1, -1)
                outs.append(o)
            return outs


class DiscriminatorAdversarialLoss:
    """losses/adversarial_loss.py DiscriminatorAdversarialLoss on the HIP path with a backward: (real_loss, fake_loss), the values
    ``discriminator.DiscriminatorAdversarialLoss`` folds; backward is adk_disc_loss_grad on every final output (kinds 0 and 1
    for mse, 4 and 5 with the sign for hinge; the coefficient holds 1 / count and the averaging)."""

    def __init__(self, average_by_discriminators=True, loss_type="mse"):
        self._plain = D.DiscriminatorAdversarialLoss(average_by_discriminators=average_by_discriminators, loss_type=loss_type)
        self.average_by_discriminators = average_by_discriminators
        self.loss_type = loss_type

    def forward(self, outputs_hat, outputs):
        is_list = D._as_list(outputs) is not None
        hats = [D._final(o) for o in outputs_hat] if is_list else [outputs_hat]
        reals = [D._final(o) for o in outputs] if is_list else [outputs]
        n = min(len(hats), len(reals))                       # zip() in the reference
        hats, reals = hats[:n], reals[:n]
        if not (torch.is_grad_enabled() and any(t.requires_grad for t in hats + reals)):
            return self._plain(outputs_hat, outputs)
        fh, fr = [D._flat(t, True) for t in hats], [D._flat(t, True) for t in reals]

        def value():
            return self._plain(fh, fr) if is_list else self._plain(fh[0], fr[0])

        (rk, rs), (fk, fs) = self._plain.kinds()
        div = n if is_list and self.average_by_discriminators else 1
        terms = [(i, a, None, rk, rs / a.numel() / div, {0: 1.0}) for i, a in enumerate(fr) if a.numel()]
        terms += [(n + i, a, None, fk, fs / a.numel() / div, {1: 1.0}) for i, a in enumerate(fh) if a.numel()]
        return D._LossFn.apply(value, terms, *[lazy_guard.plain(t) for t in reals + hats])

    __call__ = forward
