"""HiFi-GAN discriminator and the GAN eval losses on the device (adk_disc_conv, adk_disc_prep, adk_disc_loss).

Mirrors ``models/vocoder/modules/discriminator.py``: ``HiFiGANMultiScaleDiscriminator`` (lines 213-449) and
``HiFiGANMultiPeriodDiscriminator`` (lines 27-210), combined as ``models/vocoder/HiFiGAN.py:308-395`` ``Discriminator``, which
codecTrain.py:140-147 builds for the ``symAudioDec`` and ``HiFiGAN`` model types.  The losses mirror
``losses/adversarial_loss.py`` and ``losses/feat_match_loss.py``; ``AdversarialEval`` computes the four values the reference's
eval step logs (trainer/trainerGAN.py:244-268).

Every conv is one HIP call on an (N, C, H, P) tensor (P = 1 for the scale discriminator, P = period for the period
discriminator): an implicit GEMM on the f32-input MFMA, or a direct kernel for the C_in/groups = 1 first layers and the
C_out/groups = 1 output layers (chosen per layer here, see ``conv_impl``).  Exact f32 throughout.

State dicts use the reference's keys.  The scale discriminator's layers are ``nn.Conv1d``, which the reference's
``apply_weight_norm`` / ``apply_spectral_norm`` skip (they test ``isinstance(m, nn.Conv2d)``), so it has plain ``weight``
keys whatever ``follow_official_norm`` says.  The period discriminator's layers carry weight norm (``weight_g``/``weight_v``),
folded once at load as ``torch._weight_norm(v, g, 0)``.

Forward only by default: an input that requires grad while grad is enabled raises NotImplementedError.  With
``differentiable=True`` (not in the reference, whose modules always are) the discriminators, ``GeneratorAdversarialLoss``,
``FeatureMatchLoss`` and ``AdversarialEval`` give the generated waveform ``y_hat`` a gradient through ``torch.autograd``: each conv
(with its activation) and each padding / pooling step is a Function whose backward is adk_disc_conv_grad / adk_disc_prep_grad,
and each loss reduction one whose backward is adk_disc_loss_grad.  The discriminator's weights stay constants (no dW), the natural
side ``y`` may never require grad, and the backward is once-differentiable and bitwise reproducible.  A differentiable pass keeps
the ``y_hat`` feature pyramid alive until backward (the leaky masks are taken from the saved layer outputs).
``DiscriminatorAdversarialLoss`` and ``AdversarialEval.update`` stay forward only.
"""
import copy
import os
from collections import namedtuple

import torch

from . import lazy_guard, native
from .loss_common import _ptr, _settled

ACT_NONE, ACT_LEAKY = 0, 2
IMPL_DIRECT, IMPL_GEMM = 1, 2
PREP_REFLECT, PREP_AVGPOOL = 0, 1
LOSS_MSE_ONE, LOSS_SQ, LOSS_L1, LOSS_SUM, LOSS_HINGE_REAL, LOSS_HINGE_FAKE = 0, 1, 2, 3, 4, 5

# one conv layer: key = state-dict prefix of its nn.Conv (".weight" etc. follow), act_slope None = no activation,
# norm "none" | "weight" | "spectral", conv2d = a (kernel, 1) Conv2d of the period discriminator
class Layer(namedtuple("Layer", "key cin cout kernel stride pad groups bias act_slope norm conv2d")):
    """A layer description says what loading needs of it: ``weight_shape``, ``fold`` (the state dict's weight in that shape's
    rank) and ``conv``, the holder of its device weights."""
    __slots__ = ()

    @property
    def weight_shape(self):
        return (self.cout, self.cin // self.groups, self.kernel)

    def fold(self, w):
        return w.reshape(w.shape[0], w.shape[1], w.shape[2]) if self.conv2d else w

    def conv(self, w, b, dev):
        return _Conv(self, w, b, dev)


SCALE_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_sizes=[15, 41, 5, 3], channels=128, max_downsample_channels=1024,
                      max_groups=16, bias=True, downsample_scales=[2, 2, 4, 4, 1], nonlinear_activation="LeakyReLU",
                      nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, use_spectral_norm=False)
PERIOD_DEFAULTS = dict(in_channels=1, out_channels=1, period=3, kernel_sizes=[5, 3], channels=32, downsample_scales=[3, 3, 3, 3, 1],
                       max_downsample_channels=1024, bias=True, nonlinear_activation="LeakyReLU",
                       nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, use_spectral_norm=False)
MSD_DISC_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_sizes=[15, 41, 5, 3], channels=128, max_downsample_channels=1024,
                         max_groups=16, bias=True, downsample_scales=[2, 2, 4, 4, 1], nonlinear_activation="LeakyReLU",
                         nonlinear_activation_params={"negative_slope": 0.1})
MPD_DISC_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_sizes=[5, 3], channels=32, downsample_scales=[3, 3, 3, 3, 1],
                         max_downsample_channels=1024, bias=True, nonlinear_activation="LeakyReLU",
                         nonlinear_activation_params={"negative_slope": 0.1}, use_weight_norm=True, use_spectral_norm=False)
POOL_DEFAULTS = {"kernel_size": 4, "stride": 2, "padding": 2}


def _slope(nonlinear_activation, nonlinear_activation_params):
    if nonlinear_activation != "LeakyReLU":
        raise NotImplementedError(f"nonlinear_activation {nonlinear_activation!r}: the HIP discriminator implements LeakyReLU only")
    return float((nonlinear_activation_params or {}).get("negative_slope", 0.01))


def scale_layers(prefix, **kw):
    """The layers of HiFiGANScaleDiscriminator(**kw) (discriminator.py:216-343), keys under ``prefix``."""
    unknown = set(kw) - set(SCALE_DEFAULTS)
    if unknown:
        raise TypeError(f"HiFiGANScaleDiscriminator: unexpected arguments {sorted(unknown)}")
    p = dict(SCALE_DEFAULTS, **kw)
    ks = list(p["kernel_sizes"])
    assert len(ks) == 4 and all(k % 2 == 1 for k in ks)
    if p["use_weight_norm"] and p["use_spectral_norm"]:
        raise ValueError("Either use use_weight_norm or use_spectral_norm.")
    s, bias = _slope(p["nonlinear_activation"], p["nonlinear_activation_params"]), bool(p["bias"])
    out = [Layer(f"{prefix}layers.0.0.conv", p["in_channels"], p["channels"], ks[0], 1, (ks[0] - 1) // 2, 1, bias, s, "none", False)]
    in_chs = out_chs = p["channels"]
    groups = 4
    for i, ds in enumerate(p["downsample_scales"]):
        out.append(Layer(f"{prefix}layers.{i + 1}.0.conv", in_chs, out_chs, ks[1], ds, (ks[1] - 1) // 2, groups, bias, s, "none", False))
        in_chs = out_chs
        out_chs = min(in_chs * 2, p["max_downsample_channels"])
        groups = min(groups * 4, p["max_groups"])
    n = len(out)
    out_chs = min(in_chs * 2, p["max_downsample_channels"])
    out.append(Layer(f"{prefix}layers.{n}.0.conv", in_chs, out_chs, ks[2], 1, (ks[2] - 1) // 2, 1, bias, s, "none", False))
    out.append(Layer(f"{prefix}layers.{n + 1}.conv", out_chs, p["out_channels"], ks[3], 1, (ks[3] - 1) // 2, 1, bias, None, "none", False))
    return out


def period_layers(prefix, **kw):
    """The layers of HiFiGANPeriodDiscriminator(**kw) (discriminator.py:30-109), keys under ``prefix``.  NonCausalConv2d is built
    without a bias argument there, so every layer has a bias whatever ``bias`` says."""
    unknown = set(kw) - set(PERIOD_DEFAULTS)
    if unknown:
        raise TypeError(f"HiFiGANPeriodDiscriminator: unexpected arguments {sorted(unknown)}")
    p = dict(PERIOD_DEFAULTS, **kw)
    ks = list(p["kernel_sizes"])
    assert len(ks) == 2 and ks[0] % 2 == 1 and ks[1] % 2 == 1
    if p["use_weight_norm"] and p["use_spectral_norm"]:
        raise ValueError("Either use use_weight_norm or use_spectral_norm.")
    norm = "weight" if p["use_weight_norm"] else "spectral" if p["use_spectral_norm"] else "none"
    s = _slope(p["nonlinear_activation"], p["nonlinear_activation_params"])
    out = []
    in_chs, out_chs = p["in_channels"], p["channels"]
    for i, ds in enumerate(p["downsample_scales"]):
        out.append(Layer(f"{prefix}convs.{i}.0.conv", in_chs, out_chs, ks[0], ds, (ks[0] - 1) // 2, 1, True, s, norm, True))
        in_chs = out_chs
        out_chs = min(out_chs * 4, p["max_downsample_channels"])
    # output_conv: kernel (ks[1] - 1, 1), padding ((ks[1] - 1) // 2, 0): H + 1 rows for the shipped [5, 3]
    out.append(Layer(f"{prefix}output_conv.conv", out_chs, p["out_channels"], ks[1] - 1, 1, (ks[1] - 1) // 2, 1, True, None, norm, True))
    return out


def conv_out_len(h, layer):
    return (h + 2 * layer.pad - layer.kernel) // layer.stride + 1


def pool_out_len(n, kernel_size=4, stride=2, padding=2):
    """AvgPool1d(ceil_mode=False) output length; L // 2 + 1 for the reference's (4, 2, 2)."""
    return (n + 2 * padding - kernel_size) // stride + 1


def reflect_pad_len(t, period):
    """Samples the period discriminator adds on the right (discriminator.py:123-126)."""
    return 0 if t % period == 0 else period - t % period


def conv_impl(layer):
    """Kernel per layer: the direct kernel where a GEMM tile would be mostly padding (C_in/g = 1 or C_out/g = 1), else the GEMM."""
    cin_g, cout_g = layer.cin // layer.groups, layer.cout // layer.groups
    return IMPL_DIRECT if cin_g == 1 or cout_g == 1 else IMPL_GEMM


def effective_weight(sd, layer):
    """``layer.weight_shape`` float32 CPU weight of one layer from a reference state dict (weight norm folded): (C_out, C_in/g, k),
    or (C_out, C_in, kh, kw) for a spectral layer."""
    k = layer.key
    if f"{k}.weight_orig" in sd or f"{k}.weight_u" in sd:
        raise NotImplementedError(f"{k}: spectral-norm parameters (weight_orig / weight_u) are not implemented on the HIP path")
    if f"{k}.weight_g" in sd:
        w = torch._weight_norm(sd[f"{k}.weight_v"].float(), sd[f"{k}.weight_g"].float(), 0)
    else:
        w = sd[f"{k}.weight"].float()
    w = layer.fold(w.detach().cpu())
    exp = layer.weight_shape
    if tuple(w.shape) != exp:
        raise ValueError(f"{k}: weight shape {tuple(w.shape)} does not match the configured {exp}")
    return w.contiguous()


def expected_keys(layer):
    k = layer.key
    ks = [f"{k}.weight_g", f"{k}.weight_v"] if layer.norm == "weight" else [f"{k}.weight"]
    return ks + ([f"{k}.bias"] if layer.bias else [])


def _no_grad_inputs(*ts):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts):
        raise NotImplementedError("the HIP discriminator is forward only: run it under torch.no_grad() or detach the inputs")


def _wants_grad(differentiable, *ts):
    return bool(differentiable) and torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def pack_grad_weights(w, layer):
    """The backward-data GEMM's weights of one layer from its (C_out, C_in/g, k) weight: [g][phase r < stride][kk][m], where
    phase r holds the taps t = r, r + stride, ... (the only ones that reach an input row h with (h + pad) % stride == r),
    kk = co * taps(r) + tt and m = ci.  Flat (g, C_out/g * k, C_in/g): the phases of a group follow each other."""
    g, s = layer.groups, layer.stride
    cout_g, cin_g, k = layer.cout // g, layer.cin // g, layer.kernel
    w = w.reshape(g, cout_g, cin_g, k)
    phases = [w[:, :, :, r::s].permute(0, 1, 3, 2).reshape(g, -1, cin_g) for r in range(min(s, k))]
    return torch.cat(phases, 1).contiguous()


def _check_slopes(layers, differentiable):
    if differentiable and any(L.act_slope is not None and L.act_slope < 0 for L in layers):
        raise ValueError("differentiable=True needs negative_slope >= 0: the backward takes the LeakyReLU mask from the layer's output")


class _ConvBase:
    """One layer's device weights and its two native calls.  A subclass names the calls (``_native``: forward, backward) and
    gives ``_impl``, the forward GEMM packing and its inverse (``_pack``, ``_unpack``), the backward GEMM packing
    (``_pack_grad``), ``_out_shape`` and ``_geometry``, the integer arguments both calls take between the input's shape and
    ``act``."""

    def __init__(self, layer, w, b, dev):
        self.layer, self.impl = layer, self._impl(layer)
        act = ACT_LEAKY if layer.act_slope is not None else ACT_NONE
        self._tail = (*self._geometry(), act, float(layer.act_slope or 0.0))   # between the shape and impl in both calls
        self._w_grad = None                                                    # the backward's GEMM packing, made on first use
        if self.impl == IMPL_GEMM:
            w = self._pack(w)
        self.w = w.contiguous().to(dev)
        self.b = b.float().contiguous().to(dev) if b is not None else None

    def grad_weights(self):
        """The weights the backward reads: the reference's layout for the direct kernel, ``_pack_grad`` for the GEMM (re-packed
        once, on the device, from the forward packing)."""
        if self.impl != IMPL_GEMM:
            return self.w
        if self._w_grad is None:
            self._w_grad = self._pack_grad(self._unpack(self.w), self.layer)
        return self._w_grad

    def _call(self, name, p0, p1, p2, out, x_shape):
        """The native call ``name`` on its three input tensors (None for an absent one) and ``out``, for a layer input of x_shape."""
        native.check(getattr(native.lib(), name)(_ptr(p0), _ptr(p1), _ptr(p2), _ptr(out), *x_shape, *self._tail, self.impl,
                                                 native.current_stream(out.device)), name)
        return out

    def grad(self, dy, y, x_shape):
        """dy, y of the output's shape, contiguous float32 -> dx of x_shape."""
        dx = torch.empty(*x_shape, dtype=torch.float32, device=dy.device)
        return self._call(self._native[1], dy, y if self.layer.act_slope is not None else None, self.grad_weights(), dx, x_shape)

    def __call__(self, x):
        """x (N, C_in, ...) contiguous float32 -> (N, C_out, ...)."""
        y = torch.empty(*self._out_shape(x.shape), dtype=torch.float32, device=x.device)
        return self._call(self._native[0], x, self.w, self.b, y, x.shape)


class _Conv(_ConvBase):
    """One HiFi-GAN layer on (N, C, H, P)."""
    _native = ("adk_disc_conv", "adk_disc_conv_grad")
    _impl = staticmethod(conv_impl)
    _pack_grad = staticmethod(pack_grad_weights)

    def _pack(self, w):
        g = self.layer.groups
        return w.reshape(g, self.layer.cout // g, -1).permute(0, 2, 1)         # [g][cin_g * k][cout_g]

    def _unpack(self, w):
        L = self.layer
        return w.permute(0, 2, 1).reshape(L.cout, L.cin // L.groups, L.kernel)

    def _out_shape(self, x_shape):
        L = self.layer
        n, _, h, p = x_shape
        ho = conv_out_len(h, L)
        if ho < 1:
            raise ValueError(f"{L.key}: input length {h} is shorter than the kernel {L.kernel} with padding {L.pad}")
        return n, L.cout, ho, p

    def _geometry(self):
        L = self.layer
        return L.cout, L.groups, L.kernel, L.stride, L.pad


def _prep(x, rows, n_in, op, a, b=0, c=0, n_out=None):
    y = torch.empty(rows, n_out, dtype=torch.float32, device=x.device)
    native.check(native.lib().adk_disc_prep(_ptr(x), _ptr(y), rows, n_in, op, a, b, c, native.current_stream(x.device)), "adk_disc_prep")
    return y


class _ConvFn(torch.autograd.Function):
    """One conv layer (with its activation) with a backward to its input: adk_disc_conv, and adk_disc_conv_grad on the saved output."""

    @staticmethod
    def forward(ctx, x, conv):
        ctx.conv, ctx.x_shape = conv, tuple(x.shape)
        y = conv(x)
        if conv.layer.act_slope is not None:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y = ctx.saved_tensors[0] if ctx.saved_tensors else None
        return ctx.conv.grad(dy.to(torch.float32).contiguous(), y, ctx.x_shape), None


class _PrepFn(torch.autograd.Function):
    """One adk_disc_prep op on (rows, n_in) with a backward: adk_disc_prep_grad."""

    @staticmethod
    def forward(ctx, x, args):
        ctx.args = args
        rows, n_in, op, a, b, c, n_out = args
        return _prep(x, rows, n_in, op, a, b, c, n_out=n_out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        rows, n_in, op, a, b, c, n_out = ctx.args
        dy = dy.to(torch.float32).contiguous()
        dx = torch.empty(rows, n_in, dtype=torch.float32, device=dy.device)
        native.check(native.lib().adk_disc_prep_grad(_ptr(dy), _ptr(dx), rows, n_in, op, a, b, c, native.current_stream(dy.device)),
                     "adk_disc_prep_grad")
        return dx, None


def _conv_op(conv, h, grad):
    return _ConvFn.apply(h, conv) if grad else conv(h)


def _prep_op(x, rows, n_in, op, a, b=0, c=0, n_out=None, grad=False):
    if grad:
        return _PrepFn.apply(x.reshape(rows, n_in), (rows, n_in, op, a, b, c, n_out))
    return _prep(x, rows, n_in, op, a, b, c, n_out=n_out)


class _Module:
    """Device handling and state-dict loading of a set of layers, of the spectral discriminators' window buffers, and of the
    sub-discriminators (children) that compute with this module's weights."""

    def _init_layers(self, layers, device, windows=(), children=()):
        self._layers = layers
        self._window_shapes = list(windows)           # [(state-dict key, expected shape)]
        self._children = list(children)
        self._host = self._host_windows = self._convs = self._windows = None
        self._dev = torch.device(device) if device is not None else None
        if self._dev is not None:
            native.require_gpu(self._dev)

    def state_dict_keys(self):
        return [k for k, _ in self._window_shapes] + [k for L in self._layers for k in expected_keys(L)]

    def load_state_dict(self, state_dict, strict=True):
        """Reference keys (spectral-norm keys raise NotImplementedError); weight norm is folded here, once; the window buffers
        are kept as loaded."""
        sd = dict(state_dict)
        for k in sd:
            if k.endswith(".weight_orig") or k.endswith(".weight_u"):
                raise NotImplementedError(f"{k}: spectral-norm parameters are not implemented on the HIP discriminator")
        want = self.state_dict_keys()
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in set(want)]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        self._host = [(L, effective_weight(sd, L), sd[f"{L.key}.bias"] if L.bias else None) for L in self._layers]
        self._host_windows = {}
        for key, shape in self._window_shapes:
            w = sd[key].detach().float().cpu().contiguous()
            if tuple(w.shape) != shape:
                raise ValueError(f"{key}: window shape {tuple(w.shape)} does not match win_length {shape[0]}")
            self._host_windows[key] = w
        self._convs = None
        self._hand_down()
        if self._dev is not None:
            self.to(self._dev)
        return self

    def to(self, device):
        dev = torch.device(device)
        native.require_gpu(dev)
        if self._dev != dev or self._convs is None:
            self._dev = dev
            if self._host is not None:
                self._convs = {L.key: L.conv(w, b, dev) for L, w, b in self._host}
                self._windows = {k: w.to(dev) for k, w in self._host_windows.items()}
        self._share()
        return self

    def _hand_down(self):
        """Children see their own slice of the loaded weights, so each can also be called by itself."""
        for m in self._children:
            own = set(m._layers)
            m._host = [h for h in self._host if h[0] in own]
            m._host_windows = {k: self._host_windows[k] for k, _ in m._window_shapes}
            m._convs = None
            m._hand_down()

    def _share(self):
        """Children compute with this module's device tensors."""
        for m in self._children:
            m._dev, m._convs, m._windows = self._dev, self._convs, self._windows
            m._share()

    @property
    def device(self):
        return self._dev

    def _prepare_device(self, x):
        """The device this module computes on (its own, or x's / the current HIP device on first use)."""
        if self._dev is None:
            self.to(x.device if x.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
        return self._dev

    def _prepare(self, x):
        if not _wants_grad(getattr(self, "differentiable", False), x):
            _no_grad_inputs(x)
        x = _settled(x)
        if self._host is None:
            raise RuntimeError(f"{type(self).__name__}: no weights loaded (call load_state_dict first)")
        self._prepare_device(x)
        if self._convs is None:
            self.to(self._dev)
        self._share()
        if x.dim() != 3:
            raise ValueError(f"expected a (B, C, T) input, got shape {tuple(x.shape)}")
        return x.to(device=self._dev, dtype=torch.float32).contiguous()

    def forward(self, x):
        """x (B, C, T) -> the reference's list (one per sub-discriminator) of lists of per-layer device tensors."""
        outs = []
        for d, l, t, n in self.layers_of(x):
            if l == 0:
                outs.append([])
            outs[d].append(t)
        return outs

    __call__ = forward


class HiFiGANMultiScaleDiscriminator(_Module):
    """discriminator.py:346-449 on the HIP path.  Same arguments and defaults; only AvgPool1d pooling is implemented."""

    def __init__(self, scales=3, downsample_pooling="AvgPool1d", downsample_pooling_params=POOL_DEFAULTS,
                 discriminator_params=MSD_DISC_DEFAULTS, follow_official_norm=False, device=None, differentiable=False, _prefix=""):
        self.differentiable = bool(differentiable)
        if downsample_pooling != "AvgPool1d":
            raise NotImplementedError(f"downsample_pooling {downsample_pooling!r}: the HIP path implements AvgPool1d only")
        pp = dict(downsample_pooling_params)
        if pp.get("ceil_mode", False) or not pp.get("count_include_pad", True) or pp.get("divisor_override") is not None:
            raise NotImplementedError("AvgPool1d: only ceil_mode=False, count_include_pad=True, no divisor_override")
        k = int(pp["kernel_size"])
        self.pool = (k, int(pp.get("stride") or k), int(pp.get("padding", 0)))
        self.scales = int(scales)
        self.discriminator_layers = []
        for i in range(self.scales):
            params = copy.deepcopy(dict(discriminator_params))
            if follow_official_norm:                  # no effect on parameters: the layers are Conv1d (module docstring)
                params["use_weight_norm"], params["use_spectral_norm"] = (False, True) if i == 0 else (True, False)
            self.discriminator_layers.append(scale_layers(f"{_prefix}discriminators.{i}.", **params))
        _check_slopes([L for ls in self.discriminator_layers for L in ls], self.differentiable)
        self._init_layers([L for ls in self.discriminator_layers for L in ls], device)

    def layers_of(self, x, d0=0, prepared=False):
        """Yields (sub-discriminator index + d0, layer, tensor, layers of that sub-discriminator) in the reference's order, one
        layer at a time (a caller that drops each tensor never holds the whole feature pyramid)."""
        x = x if prepared else self._prepare(x)
        grad = _wants_grad(self.differentiable, x)
        b, c, t = x.shape
        cur, n = x, t
        for d, layers in enumerate(self.discriminator_layers):
            h = cur.reshape(b, c, n, 1)
            for l, L in enumerate(layers):
                h = _conv_op(self._convs[L.key], h, grad)
                yield d0 + d, l, h.reshape(h.shape[0], h.shape[1], h.shape[2]), len(layers)
            if d + 1 < len(self.discriminator_layers):
                k, s, p = self.pool
                n2 = pool_out_len(n, k, s, p)
                if n2 < 1:
                    raise ValueError(f"input length {t}: too short for {self.scales} scales")
                cur = _prep_op(cur, b * c, n, PREP_AVGPOOL, k, s, p, n_out=n2, grad=grad).reshape(b, c, n2)
                n = n2


class HiFiGANMultiPeriodDiscriminator(_Module):
    """discriminator.py:160-210 on the HIP path.  Same arguments and defaults."""

    def __init__(self, periods=[2, 3, 5, 7, 11], discriminator_params=MPD_DISC_DEFAULTS, device=None, differentiable=False,
                 _prefix=""):
        self.differentiable = bool(differentiable)
        self.periods = [int(p) for p in periods]
        self.discriminator_layers = []
        for i, period in enumerate(self.periods):
            params = copy.deepcopy(dict(discriminator_params))
            params["period"] = period
            self.discriminator_layers.append(period_layers(f"{_prefix}discriminators.{i}.", **params))
        _check_slopes([L for ls in self.discriminator_layers for L in ls], self.differentiable)
        self._init_layers([L for ls in self.discriminator_layers for L in ls], device)

    def layers_of(self, x, d0=0, prepared=False):
        x = x if prepared else self._prepare(x)
        grad = _wants_grad(self.differentiable, x)
        b, c, t = x.shape
        for d, (p, layers) in enumerate(zip(self.periods, self.discriminator_layers)):
            n_pad = reflect_pad_len(t, p)
            if n_pad >= t:
                raise ValueError(f"input length {t}: reflect padding of {n_pad} for period {p} needs more than {n_pad} samples "
                                 "(F.pad raises for it too)")
            xp = _prep_op(x, b * c, t, PREP_REFLECT, n_pad, n_out=t + n_pad, grad=grad) if n_pad else x
            h = xp.reshape(b, c, (t + n_pad) // p, p)
            for l, L in enumerate(layers):
                h = _conv_op(self._convs[L.key], h, grad)
                out = h if l + 1 < len(layers) else h.reshape(b, -1)          # torch.flatten(x, 1, -1)
                yield d0 + d, l, out, len(layers)


class Discriminator(_Module):
    """models/vocoder/HiFiGAN.py:308-395 on the HIP path: msd(x) + mpd(x), (B, C, T) with C != 1 read as (B*C, 1, T).
    Same arguments and defaults; state-dict keys ``msd.…`` and ``mpd.…`` as the reference's."""

    def __init__(self, scales=3, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=POOL_DEFAULTS,
                 scale_discriminator_params=MSD_DISC_DEFAULTS, follow_official_norm=True, periods=[2, 3, 5, 7, 11],
                 period_discriminator_params=MPD_DISC_DEFAULTS, device=None, differentiable=False):
        self.differentiable = bool(differentiable)
        self.msd = HiFiGANMultiScaleDiscriminator(scales=scales, downsample_pooling=scale_downsample_pooling,
                                                  downsample_pooling_params=scale_downsample_pooling_params,
                                                  discriminator_params=scale_discriminator_params,
                                                  follow_official_norm=follow_official_norm, differentiable=differentiable,
                                                  _prefix="msd.")
        self.mpd = HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params,
                                                   differentiable=differentiable, _prefix="mpd.")
        self.discriminator_layers = self.msd.discriminator_layers + self.mpd.discriminator_layers
        self._init_layers(self.msd._layers + self.mpd._layers, device, children=[self.msd, self.mpd])

    @property
    def n_discriminators(self):
        return len(self.discriminator_layers)

    def layers_of(self, x):
        x = self._prepare(x)
        b, c, t = x.shape
        if c != 1:
            x = x.reshape(b * c, 1, t)
        yield from self.msd.layers_of(x, 0, prepared=True)
        yield from self.mpd.layers_of(x, len(self.msd.discriminator_layers), prepared=True)


# ---- losses (losses/adversarial_loss.py, losses/feat_match_loss.py) ----
class _Terms:
    """Per-term f64 sums and element counts on the device, folded by adk_disc_loss."""

    def __init__(self, n, device):
        self.sum = torch.zeros(max(n, 1), dtype=torch.float64, device=device)
        self.count = torch.zeros(max(n, 1), dtype=torch.int64, device=device)
        self._ws = None

    def reset(self):
        self.sum.zero_()
        self.count.zero_()

    def fold(self, i, a, kind, b=None, n=None):
        """sum[i] += sum of the term over the first n elements of a (and b); count[i] += n."""
        n = a.numel() if n is None else int(n)
        lib = native.lib()
        ws_bytes = int(lib.adk_disc_loss_workspace_bytes(n))
        if ws_bytes < 0:
            native.check(ws_bytes, "adk_disc_loss_workspace_bytes")
        if ws_bytes and (self._ws is None or self._ws.numel() * 8 < ws_bytes):
            self._ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=self.sum.device)
        native.check(lib.adk_disc_loss(_ptr(a), _ptr(b), n, kind, _ptr(self.sum[i:i + 1]), _ptr(self.count[i:i + 1]),
                                       _ptr(self._ws) if ws_bytes else None, None, native.current_stream(self.sum.device)),
                     "adk_disc_loss")

    def means(self):
        """(sum / count) per term, float64 on the device (NaN where nothing was folded)."""
        return self.sum / self.count.to(torch.float64)


class _LossFn(torch.autograd.Function):
    """Loss values with a backward to the generated side's tensors.  ``value()`` returns the tuple of 0-d float32 values (the
    forward-only code's); ``terms`` is a list of (input index, a, b, kind, coef, weights): the term contributes
    coef * sum_i term(a[i], b[i]) to the outputs k of weights = {k: factor}, scaled by factor.  backward: per term
    adk_disc_loss_grad with the upstream sum_k factor_k g_k, formed and read on the device; terms of one input are added in order."""

    @staticmethod
    def forward(ctx, value, terms, *hats):
        ctx.terms, ctx.like = terms, [(h.shape, h.device, h.dtype) for h in hats]
        return value()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        grads = [None] * len(ctx.like)
        lib = native.lib()
        for i, a, b, kind, coef, weights in ctx.terms:
            if not ctx.needs_input_grad[2 + i]:
                continue
            up = None
            for k, f in weights.items():
                g = gs[k].reshape(1).to(device=a.device, dtype=torch.float32)
                g = g if f == 1.0 else g * f
                up = g if up is None else up + g
            out = torch.empty_like(a)
            native.check(lib.adk_disc_loss_grad(_ptr(a), _ptr(b), a.numel(), kind, float(coef), _ptr(up.contiguous()), _ptr(out),
                                                native.current_stream(a.device)), "adk_disc_loss_grad")
            grads[i] = out if grads[i] is None else grads[i] + out
        res = []
        for g, (shape, device, dtype) in zip(grads, ctx.like):
            res.append(None if g is None else g.reshape(shape).to(device=device, dtype=dtype))
        return (None, None, *res)


def _final(o):
    return o[-1] if isinstance(o, (tuple, list)) else o


def _flat(t, grad_ok=False):
    t = _settled(t)
    if not grad_ok:
        _no_grad_inputs(t)
    return t.detach().to(torch.float32).contiguous()


def _check_loss_type(loss_type):
    assert loss_type in ["mse", "hinge"], f"{loss_type} is not supported."


def _as_list(outputs):
    return list(outputs) if isinstance(outputs, (tuple, list)) else None


class GeneratorAdversarialLoss:
    """losses/adversarial_loss.py GeneratorAdversarialLoss on the HIP path: sum (or mean) over discriminators of
    mse(D(y_hat), 1) or -mean(D(y_hat)); each discriminator's final output is reduced by adk_disc_loss."""

    def __init__(self, average_by_discriminators=True, loss_type="mse", differentiable=False):
        _check_loss_type(loss_type)
        self.average_by_discriminators = average_by_discriminators
        self.loss_type = loss_type
        self.differentiable = bool(differentiable)

    def kind(self):
        return (LOSS_MSE_ONE, 1.0) if self.loss_type == "mse" else (LOSS_SUM, -1.0)

    def coef(self, count, n_discriminators):
        """d loss / d (sum of the term over one discriminator's final output of `count` elements)."""
        return self.kind()[1] / count / (n_discriminators if self.average_by_discriminators else 1)

    def forward(self, outputs):
        outs = _as_list(outputs)
        outs = [_final(o) for o in outs] if outs is not None else [outputs]
        grad = _wants_grad(self.differentiable, *outs)
        ts = [_flat(o, grad) for o in outs]
        averaged = _as_list(outputs) is not None and self.average_by_discriminators

        def value():
            terms = _Terms(len(ts), ts[0].device)
            kind, sign = self.kind()
            for i, t in enumerate(ts):
                terms.fold(i, t, kind)
            v = terms.means().sum() * sign
            if averaged:
                v = v / len(ts)
            return v.to(torch.float32)

        if not grad:
            return value()
        terms = [(i, t, None, self.kind()[0], self.kind()[1] / t.numel() / (len(ts) if averaged else 1), {0: 1.0})
                 for i, t in enumerate(ts) if t.numel()]
        return _LossFn.apply(lambda: (value(),), terms, *[lazy_guard.plain(o) for o in outs])[0]

    __call__ = forward


class DiscriminatorAdversarialLoss:
    """losses/adversarial_loss.py DiscriminatorAdversarialLoss on the HIP path: (real_loss, fake_loss)."""

    def __init__(self, average_by_discriminators=True, loss_type="mse"):
        _check_loss_type(loss_type)
        self.average_by_discriminators = average_by_discriminators
        self.loss_type = loss_type

    def kinds(self):
        """((real kind, sign), (fake kind, sign))"""
        if self.loss_type == "mse":
            return (LOSS_MSE_ONE, 1.0), (LOSS_SQ, 1.0)
        return (LOSS_HINGE_REAL, -1.0), (LOSS_HINGE_FAKE, -1.0)

    def forward(self, outputs_hat, outputs):
        is_list = _as_list(outputs) is not None
        hats = [_flat(_final(o)) for o in outputs_hat] if is_list else [_flat(outputs_hat)]
        reals = [_flat(_final(o)) for o in outputs] if is_list else [_flat(outputs)]
        n = min(len(hats), len(reals))                       # zip() in the reference
        terms = _Terms(2 * n, reals[0].device)
        (rk, rs), (fk, fs) = self.kinds()
        for i in range(n):
            terms.fold(2 * i, reals[i], rk)
            terms.fold(2 * i + 1, hats[i], fk)
        m = terms.means()
        real, fake = m[0:2 * n:2].sum() * rs, m[1:2 * n:2].sum() * fs
        if is_list and self.average_by_discriminators:
            real, fake = real / n, fake / n
        return real.to(torch.float32), fake.to(torch.float32)

    __call__ = forward


class FeatureMatchLoss:
    """losses/feat_match_loss.py FeatureMatchLoss on the HIP path: per discriminator the sum (or mean) over layers of
    F.l1_loss(feat_hat, feat), summed (or averaged) over discriminators."""

    def __init__(self, average_by_layers=True, average_by_discriminators=True, include_final_outputs=False, differentiable=False):
        self.average_by_layers = average_by_layers
        self.average_by_discriminators = average_by_discriminators
        self.include_final_outputs = include_final_outputs
        self.differentiable = bool(differentiable)

    def layers_used(self, n_layers):
        return n_layers if self.include_final_outputs else n_layers - 1

    def combine(self, means, layout):
        """means: f64 per (discriminator, layer) term in the order of layout = [layers used per discriminator]."""
        total, i = None, 0
        for n in layout:
            v = means[i:i + n].sum()
            if self.average_by_layers and n:
                v = v / n
            total = v if total is None else total + v
            i += n
        if self.average_by_discriminators and layout:
            total = total / len(layout)
        return total

    def coefs(self, counts, layout):
        """d loss / d (sum of |a - b| over one used feature map), in the order of the terms: counts = elements per term."""
        out, i = [], 0
        for n in layout:
            for c in counts[i:i + n]:
                out.append(1.0 / c / (n if self.average_by_layers else 1) / (len(layout) if self.average_by_discriminators else 1))
            i += n
        return out

    def forward(self, feats_hat, feats):
        raw, layout = [], []
        for fh, f in zip(feats_hat, feats):
            fh, f = list(fh), list(f)
            if not self.include_final_outputs:
                fh, f = fh[:-1], f[:-1]
            used = list(zip(fh, f))
            layout.append(len(used))
            raw += used
        grad = _wants_grad(self.differentiable, *[a for a, _ in raw])
        pairs = []
        for a, b in raw:
            a, b = _flat(a, grad), _flat(b)
            if a.shape != b.shape:
                raise ValueError(f"feature shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
            pairs.append((a, b))

        def value():
            terms = _Terms(len(pairs), pairs[0][0].device)
            for i, (a, b) in enumerate(pairs):
                terms.fold(i, a, LOSS_L1, b)
            return self.combine(terms.means(), layout).to(torch.float32)

        if not grad:
            return value()
        coefs = self.coefs([a.numel() for a, _ in pairs], layout)
        terms = [(i, a, b, LOSS_L1, coefs[i], {0: 1.0}) for i, (a, b) in enumerate(pairs) if a.numel()]
        return _LossFn.apply(lambda: (value(),), terms, *[lazy_guard.plain(a) for a, _ in raw])[0]

    __call__ = forward


class AdversarialEval:
    """The four GAN values of the reference's eval step (trainer/trainerGAN.py:244-268) for a generator output y_hat and its
    target y, from ONE discriminator pass over cat([y_hat, y]):

      adversarial_loss       lambda_adv * (gen_adv(D(y_hat)) + lambda_feat_match * feature_matching_loss)
      feature_matching_loss  feat_match(D(y_hat), D(y))   (only when use_feat_match_loss; else the key is absent)
      real_loss, fake_loss   dis_adv(D(y_hat), D(y))

    Each layer's feature-matching term is folded as soon as the layer is produced and the layer is dropped, so the feature
    pyramid is never held whole.  ``forward(y_hat, y)`` returns 0-d float32 device tensors for one batch without synchronising;
    ``update(y_hat, y)`` folds a batch into device-side totals and ``value()`` returns the values of all folded batches as one
    batch (floats; synchronises), like mel.MelDistance; ``reset()`` zeroes the totals.

    ``differentiable=True`` (with a discriminator built with it too): ``forward(y_hat, y)`` with a ``y_hat`` that requires grad runs
    D(y) under no_grad and D(y_hat) with the graph, as the reference's generator step does (trainer/autoencoder.py:102-108);
    ``adversarial_loss`` and ``feature_matching_loss`` then carry grad, ``real_loss`` and ``fake_loss`` are plain values, and all
    four equal the forward-only call's.  That pass holds both feature pyramids until the losses are folded and the ``y_hat`` one
    until backward.  ``y`` may never require grad; ``update()`` stays forward only."""

    def __init__(self, discriminator, generator_adv_loss_params=None, discriminator_adv_loss_params=None,
                 use_feat_match_loss=True, feat_match_loss_params=None, lambda_adv=1.0, lambda_feat_match=2.0,
                 differentiable=False):
        self.discriminator = discriminator
        self.differentiable = bool(differentiable)
        self.gen_adv = GeneratorAdversarialLoss(**dict(generator_adv_loss_params or {}))
        self.dis_adv = DiscriminatorAdversarialLoss(**dict(discriminator_adv_loss_params or {}))
        self.feat_match = FeatureMatchLoss(**dict(feat_match_loss_params or {})) if use_feat_match_loss else None
        self.lambda_adv, self.lambda_feat_match = float(lambda_adv), float(lambda_feat_match)
        self._totals = None

    def _layout(self):
        subs = self.discriminator.discriminator_layers
        fm = [self.feat_match.layers_used(len(ls)) for ls in subs] if self.feat_match else []
        return len(subs), fm

    def _new_terms(self, dev):
        n_d, fm = self._layout()
        return _Terms(3 * n_d + sum(fm), dev)

    @staticmethod
    def _waveforms(y_hat, y):
        """Both settled and of one shape, (B, T) read as (B, 1, T)."""
        y_hat, y = _settled(y_hat), _settled(y)
        if tuple(y_hat.shape) != tuple(y.shape):
            raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} must have the same shape")
        if y.dim() == 2:
            y_hat, y = y_hat[:, None], y[:, None]
        return y_hat, y

    def _fm_used(self, last):
        return self.feat_match is not None and (not last or self.feat_match.include_final_outputs)

    def _plan(self):
        """Where the terms of a pass go and of which kind they are, once per pass: (the first feature-matching term of each
        sub-discriminator, the generator's kind, the real and fake kinds)."""
        n_d, fm = self._layout()
        (rk, _), (fk, _) = self.dis_adv.kinds()
        return [3 * n_d + sum(fm[:d]) for d in range(n_d)], self.gen_adv.kind()[0], rk, fk

    def _fold_layer(self, terms, plan, d, l, last, a, b, n=None):
        """Folds layer l of sub-discriminator d: the first n elements of a (the y_hat side) and b (the y side) into its
        feature-matching term and, for the final output, the three adversarial terms."""
        fm_off, gk, rk, fk = plan
        if self._fm_used(last):
            terms.fold(fm_off[d] + l, a, LOSS_L1, b, n=n)
        if last:
            terms.fold(3 * d, a, gk, n=n)
            terms.fold(3 * d + 1, b, rk, n=n)
            terms.fold(3 * d + 2, a, fk, n=n)

    def _fold(self, terms, y_hat, y):
        _no_grad_inputs(y_hat, y)
        y_hat, y = self._waveforms(y_hat, y)
        x = torch.cat([y_hat.to(terms.sum.device, torch.float32), y.to(terms.sum.device, torch.float32)], 0)
        plan = self._plan()
        for d, l, t, n_layers in self.discriminator.layers_of(x):
            half = t.numel() // 2                         # rows [0, B) are y_hat, rows [B, 2B) are y
            self._fold_layer(terms, plan, d, l, l == n_layers - 1, t, t.view(-1)[half:], n=half)
            del t

    def _combine(self, means):
        n_d, fm = self._layout()
        _, gs = self.gen_adv.kind()
        (_, rs), (_, fs) = self.dis_adv.kinds()
        adv, real, fake = means[0:3 * n_d:3].sum() * gs, means[1:3 * n_d:3].sum() * rs, means[2:3 * n_d:3].sum() * fs
        if self.gen_adv.average_by_discriminators:
            adv = adv / n_d
        if self.dis_adv.average_by_discriminators:
            real, fake = real / n_d, fake / n_d
        out = {}
        if self.feat_match is not None:
            fmv = self.feat_match.combine(means[3 * n_d:], fm)
            out["feature_matching_loss"] = fmv
            adv = adv + self.lambda_feat_match * fmv
        out["adversarial_loss"] = adv * self.lambda_adv
        out["real_loss"], out["fake_loss"] = real, fake
        return out

    def _forward_grad(self, dev, y_hat, y):
        _no_grad_inputs(y)
        y_hat, y = self._waveforms(y_hat, y)
        with torch.no_grad():
            real = [_flat(t) for _, _, t, _ in self.discriminator.layers_of(y)]
        hats, where = [], []
        for d, l, t, n_layers in self.discriminator.layers_of(y_hat):
            hats.append(t)
            where.append((d, l, l == n_layers - 1))
        flat = [_flat(t, True) for t in hats]
        n_d, fm = self._layout()
        plan, plain = self._plan(), {}

        def value():
            terms = self._new_terms(dev)
            for (d, l, last), a, b in zip(where, flat, real):
                self._fold_layer(terms, plan, d, l, last, a, b)
            plain.update({k: v.to(torch.float32) for k, v in self._combine(terms.means()).items()})
            return tuple(plain[k] for k in ("adversarial_loss", "feature_matching_loss") if k in plain)

        used = [self._fm_used(last) for _, _, last in where]
        fm_coefs = iter(self.feat_match.coefs([a.numel() for a, u in zip(flat, used) if u], fm)) if self.feat_match else None
        gk = plan[1]
        terms = []
        for i, ((d, l, last), a, b, fm_term) in enumerate(zip(where, flat, real, used)):
            if fm_term:
                terms.append((i, a, b, LOSS_L1, next(fm_coefs), {0: self.lambda_adv * self.lambda_feat_match, 1: 1.0}))
            if last:
                terms.append((i, a, None, gk, self.gen_adv.coef(a.numel(), n_d) * self.lambda_adv, {0: 1.0}))
        out = _LossFn.apply(value, terms, *hats)
        res = dict(plain)
        res["adversarial_loss"] = out[0]
        if self.feat_match is not None:
            res["feature_matching_loss"] = out[1]
        return res

    def forward(self, y_hat, y):
        dev = self.discriminator._prepare_device(y)
        if _wants_grad(self.differentiable, y_hat):
            return self._forward_grad(dev, y_hat, y)
        terms = self._new_terms(dev)
        self._fold(terms, y_hat, y)
        return {k: v.to(torch.float32) for k, v in self._combine(terms.means()).items()}

    __call__ = forward

    def update(self, y_hat, y):
        dev = self.discriminator._prepare_device(y)
        if self._totals is None:
            self._totals = self._new_terms(dev)
        if y.shape[0] == 0:
            return self
        self._fold(self._totals, y_hat, y)
        return self

    def reset(self):
        if self._totals is not None:
            self._totals.reset()
        return self

    def value(self):
        if self._totals is None:
            return None
        return {k: float(v) for k, v in self._combine(self._totals.means()).items()}


def from_config(config, discriminator, differentiable=False):
    """AdversarialEval with a training config's loss settings (codecTrain.py:190-201, trainer/trainerGAN.py:244-268)."""
    return AdversarialEval(discriminator,
                           generator_adv_loss_params=config.get("generator_adv_loss_params", {}),
                           discriminator_adv_loss_params=config.get("discriminator_adv_loss_params", {}),
                           use_feat_match_loss=config.get("use_feat_match_loss", False),
                           feat_match_loss_params=config.get("feat_match_loss_params", {}),
                           lambda_adv=config.get("lambda_adv", 1.0), lambda_feat_match=config.get("lambda_feat_match", 1.0),
                           differentiable=differentiable)


def discriminator_for(model_type, discriminator_params, device=None):
    """codecTrain.py:140-147: the HiFi-GAN discriminator for symAudioDec / HiFiGAN; UnivNet's is not implemented."""
    if model_type in ("symAudioDec", "HiFiGAN"):
        return Discriminator(**dict(discriminator_params or {}), device=device)
    if model_type in ("symAudioDecUniv", "UnivNet"):
        raise NotImplementedError(f"Model type: {model_type} is not supported for the discriminator! "
                                  "(the UnivNet discriminator is not implemented on the HIP path)")
    raise NotImplementedError(f"Model type: {model_type} is not supported for the discriminator!")


def load_discriminator(checkpoint, device=None, discriminator_for=discriminator_for):
    """The discriminator of a training checkpoint: config.yml next to it, torch.load(checkpoint)['model']['discriminator']
    (trainer/trainerGAN.py:95-121), built by ``discriminator_for`` (this module's: the HiFi-GAN model types only).  The returned
    module's ``config`` is the parsed config.yml."""
    import yaml
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(checkpoint)), "config.yml")
    with open(cfg_path) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    disc = discriminator_for(config.get("model_type", "symAudioDec"), config.get("discriminator_params", {}), device=device)
    state = torch.load(checkpoint, map_location="cpu", weights_only=False)
    disc.load_state_dict(state["model"]["discriminator"])
    disc.config = config
    return disc
