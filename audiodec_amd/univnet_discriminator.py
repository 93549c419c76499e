"""UnivNet discriminator on the device: multi-resolution spectral + multi-period (adk_spectrogram, adk_conv2d, adk_disc_*).

Mirrors ``models/vocoder/modules/discriminator.py``: ``UnivNetSpectralDiscriminator`` (lines 451-582) and
``UnivNetMultiResolutionSpectralDiscriminator`` (lines 585-640), combined with the multi-period discriminator as
``models/vocoder/UnivNet.py:23-103`` ``Discriminator``, which codecTrain.py builds for the ``symAudioDecUniv`` and ``UnivNet``
model types.  The period half is ``discriminator.HiFiGANMultiPeriodDiscriminator`` unchanged, and the loss classes,
``AdversarialEval`` and ``from_config`` of ``discriminator`` work on this module's ``Discriminator`` as they are.

A spectral discriminator is one magnitude spectrogram (``torchaudio.functional.spectrogram`` with ``pad = win_length // 2``,
``power = 1``, transposed to (frames, bins)) and six 2-D convs over that plane, each one HIP call: an implicit GEMM on the
f32-input MFMA, or a direct kernel for the C_in = 1 first layer and the C_out = 1 output layer.  Exact f32 throughout.

State dicts use the reference's keys, including the persistent ``window`` buffer of every spectral discriminator; the
spectrogram uses the loaded window.  Weight norm (``weight_g``/``weight_v``) is folded once at load as
``torch._weight_norm(v, g, 0)``.

Forward only by default: an input that requires grad while grad is enabled raises NotImplementedError.  The classes above take
no ``differentiable`` argument; the backward to the input arrives as subclasses with the same arguments and state-dict keys,
``DifferentiableSpectralDiscriminator``, ``DifferentiableMultiResolutionSpectralDiscriminator`` and
``DifferentiableDiscriminator`` (``discriminator_for`` / ``load_discriminator`` build them with ``differentiable=True``).  With an
input that requires grad they give it a gradient through ``torch.autograd``: the spectrogram is a Function whose backward is
adk_spectrogram_grad (a bin of magnitude 0 passes no gradient, as torch's ``abs``), each 2-D conv with its activation is
``discriminator._ConvFn`` with adk_conv2d_grad behind it, and the period half is built with ``differentiable=True``.  The weights
stay constants, the backward is once-differentiable and bitwise reproducible, and without grad wanted they run the plain forward.
"""
import copy
import functools
from collections import namedtuple

import torch

from . import discriminator as D
from . import native
from .discriminator import (ACT_LEAKY, ACT_NONE, IMPL_DIRECT, IMPL_GEMM, MPD_DISC_DEFAULTS, AdversarialEval,  # noqa: F401
                            DiscriminatorAdversarialLoss, FeatureMatchLoss, GeneratorAdversarialLoss, _Module, _ptr,
                            effective_weight, expected_keys, from_config)

GEMM_MAX_K = 4096                                     # adk_conv2d impl 2: c_in * kh * kw
GRAD_GEMM_MAX_K = 4096                                # adk_conv2d_grad impl 2: c_out * kh * kw


# one 2-D conv layer: kernel, stride, pad are (frames axis, bins axis); norm "none" | "weight"
class SpecLayer(namedtuple("SpecLayer", "key cin cout kernel stride pad bias act_slope norm")):
    __slots__ = ()

    @property
    def weight_shape(self):
        return (self.cout, self.cin) + tuple(self.kernel)

    def fold(self, w):
        return w

    def conv(self, w, b, dev):
        return _Conv2d(self, w, b, dev)


SPECTRAL_DEFAULTS = dict(kernel_sizes=[(3, 9), (3, 9), (3, 9), (3, 9), (3, 3), (3, 3)],
                         strides=[(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)], channels=32, bias=True,
                         nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2},
                         use_weight_norm=True)
MRSD_DISC_DEFAULTS = dict(channels=32, kernel_sizes=[(3, 9), (3, 9), (3, 9), (3, 9), (3, 3), (3, 3)],
                          strides=[(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)], bias=True,
                          nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2})


def _pair(v, what):
    v = (v, v) if isinstance(v, int) else tuple(int(a) for a in v)
    if len(v) != 2 or min(v) < 1:
        raise ValueError(f"{what}: expected an int or a pair of positive ints, got {v!r}")
    return v


def spectral_layers(prefix, **kw):
    """The layers of UnivNetSpectralDiscriminator(**kw) (discriminator.py:490-548), keys under ``prefix``.  NonCausalConv2d
    pads (k - 1) // 2 on each axis (layers/conv_layer.py:221-224)."""
    unknown = set(kw) - set(SPECTRAL_DEFAULTS)
    if unknown:
        raise TypeError(f"UnivNetSpectralDiscriminator: unexpected arguments {sorted(unknown)}")
    p = dict(SPECTRAL_DEFAULTS, **kw)
    slope = D._slope(p["nonlinear_activation"], p["nonlinear_activation_params"])
    ks = [_pair(k, "kernel_sizes") for k in p["kernel_sizes"]]
    st = [_pair(s, "strides") for s in p["strides"]]
    assert len(ks) == len(st) and len(ks) >= 3
    ch, bias, norm = int(p["channels"]), bool(p["bias"]), "weight" if p["use_weight_norm"] else "none"
    n = len(ks)
    out = []
    for i in range(n):
        last = i == n - 1
        key = f"{prefix}layers.{i}.conv" if last else f"{prefix}layers.{i}.0.conv"
        pad = ((ks[i][0] - 1) // 2, (ks[i][1] - 1) // 2)
        out.append(SpecLayer(key, 1 if i == 0 else ch, 1 if last else ch, ks[i], st[i], pad, bias, None if last else slope, norm))
    return out


def conv2d_out_shape(h, w, layer):
    return ((h + 2 * layer.pad[0] - layer.kernel[0]) // layer.stride[0] + 1,
            (w + 2 * layer.pad[1] - layer.kernel[1]) // layer.stride[1] + 1)


def spectrogram_shape(t, fft_size, hop_size, win_length):
    """(frames, bins) of the transposed spectrogram of t samples: pad = win_length // 2 zeros on both sides, centred frames."""
    return 1 + (t + 2 * (win_length // 2)) // hop_size, fft_size // 2 + 1


def min_samples(fft_size, win_length):
    """The shortest input torch.stft's reflect padding of fft_size // 2 accepts after the zero padding."""
    return max(1, fft_size // 2 - 2 * (win_length // 2) + 1)


def conv_impl(layer):
    """Kernel per layer: the direct kernel where a GEMM tile would be mostly padding (C_in = 1 or C_out = 1), else the GEMM."""
    return IMPL_DIRECT if layer.cin == 1 or layer.cout == 1 else IMPL_GEMM


def pack_grad_weights2d(w, layer):
    """The backward-data GEMM's weights of one spectral layer from its (C_out, C_in, kh, kw) weight: [phase][kk][m], phases
    (rh, rw) with rh < stride_h major and rw < stride_w minor.  Phase (rh, rw) holds the taps th = rh, rh + stride_h, ... and
    tw = rw, rw + stride_w, ... (the only ones that reach an input position with (h + pad_h) % stride_h == rh and
    (w + pad_w) % stride_w == rw), kk = (co * taps(rh) + tth) * taps(rw) + ttw and m = ci.  Flat (C_out * kh * kw, C_in): the
    phases follow each other, one without taps takes no rows."""
    (kh, kw), (sh, sw) = layer.kernel, layer.stride
    w = w.reshape(layer.cout, layer.cin, kh, kw)
    phases = [w[:, :, rh::sh, rw::sw].permute(0, 2, 3, 1).reshape(-1, layer.cin)
              for rh in range(min(sh, kh)) for rw in range(min(sw, kw))]
    return torch.cat(phases, 0).contiguous()


def _check_grad_layers(layers):
    """What a differentiable spectral discriminator needs of its layers beyond discriminator._check_slopes."""
    for L in layers:
        kg = L.cout * L.kernel[0] * L.kernel[1]
        if conv_impl(L) == IMPL_GEMM and kg > GRAD_GEMM_MAX_K:
            raise NotImplementedError(f"{L.key}: C_out * kh * kw = {kg} is beyond the HIP 2-D conv backward's {GRAD_GEMM_MAX_K}")


class _Conv2d(D._ConvBase):
    """One spectral layer on (N, C, H, W)."""
    _native = ("adk_conv2d", "adk_conv2d_grad")
    _impl = staticmethod(conv_impl)
    _pack_grad = staticmethod(pack_grad_weights2d)

    def _pack(self, w):
        layer = self.layer
        kg = layer.cin * layer.kernel[0] * layer.kernel[1]
        if kg > GEMM_MAX_K:
            raise NotImplementedError(f"{layer.key}: C_in * kh * kw = {kg} is beyond the HIP 2-D conv's {GEMM_MAX_K}")
        return w.reshape(layer.cout, kg).t()                                    # [cin * kh * kw][cout]

    def _unpack(self, w):
        return w.t().reshape(self.layer.weight_shape)

    def _out_shape(self, x_shape):
        L = self.layer
        n, _, h, w = x_shape
        ho, wo = conv2d_out_shape(h, w, L)
        if ho < 1 or wo < 1:
            raise ValueError(f"{L.key}: input plane {h} x {w} is smaller than the kernel {L.kernel} with padding {L.pad}")
        return n, L.cout, ho, wo

    def _geometry(self):
        L = self.layer
        return (L.cout, *L.kernel, *L.stride, *L.pad)


def spectrogram(x, window, fft_size, hop_size, win_length):
    """Rows of x (N, T) float32 on the device -> (N, frames, fft_size // 2 + 1): the reference's transposed magnitude
    spectrogram (discriminator.py:557-566) through adk_spectrogram."""
    n, t = x.shape
    _check_length(t, [(None, fft_size, hop_size, win_length)])
    frames, bins = spectrogram_shape(t, fft_size, hop_size, win_length)
    out = torch.empty(n, frames, bins, dtype=torch.float32, device=x.device)
    native.check(native.lib().adk_spectrogram(_ptr(x), n, t, win_length // 2, fft_size, hop_size, _ptr(window), win_length,
                                              _ptr(out), native.current_stream(x.device)), "adk_spectrogram")
    return out


class _SpecFn(torch.autograd.Function):
    """spectrogram() with a backward to the signal: adk_spectrogram_grad on the saved input (the frames are recomputed)."""

    @staticmethod
    def forward(ctx, x, window, fft_size, hop_size, win_length):
        ctx.args = (window, fft_size, hop_size, win_length)
        ctx.save_for_backward(x)
        return spectrogram(x, window, fft_size, hop_size, win_length)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        window, fft_size, hop_size, win_length = ctx.args
        n, t = x.shape
        g = g.to(torch.float32).contiguous()
        lib = native.lib()
        ws_bytes = int(lib.adk_spectrogram_grad_workspace_bytes(n, t, win_length // 2, fft_size, hop_size))
        if ws_bytes < 0:
            native.check(ws_bytes, "adk_spectrogram_grad_workspace_bytes")
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=x.device)
        dx = torch.empty(n, t, dtype=torch.float32, device=x.device)
        native.check(lib.adk_spectrogram_grad(_ptr(x), _ptr(g), n, t, win_length // 2, fft_size, hop_size, _ptr(window), win_length,
                                              _ptr(ws), _ptr(dx), native.current_stream(x.device)), "adk_spectrogram_grad")
        return dx, None, None, None, None


def _window_shapes(specs):
    """discriminator._Module's window list of specs = [(window key, fft_size, hop_size, win_length)]."""
    return [(key, (win,)) for key, _, _, win in specs]


def _check_window(window):
    if window != "hann_window":
        raise NotImplementedError(f"window {window!r}: the HIP spectral discriminator implements hann_window only")


def _check_length(t, specs):
    for _, fft, _, win in specs:
        if t < min_samples(fft, win):
            raise ValueError(f"input length {t}: the {fft}-point spectrogram's reflect padding of {fft // 2} needs more than "
                             f"{fft // 2 - 2 * (win // 2)} samples (torch.stft raises for it too)")


def _check_fft(fft_size, hop_size, win_length):
    if fft_size < 256 or fft_size > 4096 or fft_size & (fft_size - 1):
        raise NotImplementedError(f"fft_size {fft_size}: the HIP spectrogram implements powers of two in [256, 4096]")
    if not 0 < win_length <= fft_size or hop_size < 1:
        raise ValueError(f"need 0 < win_length <= fft_size and hop_size > 0, got win_length {win_length}, hop_size {hop_size}")


class UnivNetSpectralDiscriminator(_Module):
    """discriminator.py:451-582 on the HIP path.  Same arguments and defaults."""

    def __init__(self, fft_size, hop_size, win_length, window="hann_window",
                 kernel_sizes=[(3, 9), (3, 9), (3, 9), (3, 9), (3, 3), (3, 3)],
                 strides=[(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)], channels=32, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2}, use_weight_norm=True,
                 device=None, _prefix=""):
        _check_window(window)
        self.fft_size, self.hop_size, self.win_length = int(fft_size), int(hop_size), int(win_length)
        _check_fft(self.fft_size, self.hop_size, self.win_length)
        self.window_key = f"{_prefix}window"
        self.layers = spectral_layers(_prefix, kernel_sizes=kernel_sizes, strides=strides, channels=channels, bias=bias,
                                      nonlinear_activation=nonlinear_activation,
                                      nonlinear_activation_params=nonlinear_activation_params, use_weight_norm=use_weight_norm)
        self.discriminator_layers = [self.layers]
        self._specs = [(self.window_key, self.fft_size, self.hop_size, self.win_length)]
        self._init_layers(list(self.layers), device, windows=_window_shapes(self._specs))

    def output_shapes(self, n, t):
        """Shapes of the per-layer outputs for an (n, 1, t) input."""
        h, w = spectrogram_shape(t, self.fft_size, self.hop_size, self.win_length)
        out = []
        for L in self.layers:
            h, w = conv2d_out_shape(h, w, L)
            out.append((n, L.cout, h, w))
        return out

    def layers_of(self, x, d0=0, prepared=False):
        """Yields (d0, layer, tensor, n_layers) one layer at a time."""
        if not prepared:
            x = self._prepare(x)
            if x.shape[1] != 1:
                raise ValueError(f"expected a (B, 1, T) input, got {tuple(x.shape)}")
            _check_length(x.shape[2], self._specs)
        grad = D._wants_grad(getattr(self, "differentiable", False), x)
        b, _, t = x.shape
        args = (x.reshape(b, t), self._windows[self.window_key], self.fft_size, self.hop_size, self.win_length)
        h = _SpecFn.apply(*args) if grad else spectrogram(*args)
        h = h.reshape(b, 1, h.shape[1], h.shape[2])
        for l, L in enumerate(self.layers):
            h = D._conv_op(self._convs[L.key], h, grad)
            yield d0, l, h, len(self.layers)


class UnivNetMultiResolutionSpectralDiscriminator(_Module):
    """discriminator.py:585-640 on the HIP path.  Same arguments and defaults."""
    _spectral_class = UnivNetSpectralDiscriminator

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
                 discriminator_params=MRSD_DISC_DEFAULTS, device=None, _prefix=""):
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.discriminators = []
        for i in range(len(fft_sizes)):
            params = copy.deepcopy(dict(discriminator_params))
            self.discriminators.append(self._spectral_class(fft_size=fft_sizes[i], hop_size=hop_sizes[i], win_length=win_lengths[i],
                                                            window=window, _prefix=f"{_prefix}discriminators.{i}.", **params))
        self.discriminator_layers = [d.layers for d in self.discriminators]
        self._specs = [s for d in self.discriminators for s in d._specs]
        self._init_layers([L for ls in self.discriminator_layers for L in ls], device, windows=_window_shapes(self._specs),
                          children=self.discriminators)

    def layers_of(self, x, d0=0, prepared=False):
        if not prepared:
            x = self._prepare(x)
            if x.shape[1] != 1:
                raise ValueError(f"expected a (B, 1, T) input, got {tuple(x.shape)}")
            _check_length(x.shape[2], self._specs)
        for i, d in enumerate(self.discriminators):
            yield from d.layers_of(x, d0 + i, prepared=True)


class Discriminator(_Module):
    """models/vocoder/UnivNet.py:23-103 on the HIP path: mrsd(x) + mpd(x).  Same arguments and defaults; state-dict keys
    ``mrsd.…`` (with the ``window`` buffers) and ``mpd.…`` as the reference's."""
    _spectral_half_class = UnivNetMultiResolutionSpectralDiscriminator
    _period_half_differentiable = False

    def __init__(self, fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
                 spectral_discriminator_params=MRSD_DISC_DEFAULTS, periods=[2, 3, 5, 7, 11],
                 period_discriminator_params=MPD_DISC_DEFAULTS, flat_channel=False, device=None):
        self.flat_channel = bool(flat_channel)
        self.mrsd = self._spectral_half_class(fft_sizes=fft_sizes, hop_sizes=hop_sizes, win_lengths=win_lengths, window=window,
                                              discriminator_params=spectral_discriminator_params, _prefix="mrsd.")
        self.mpd = D.HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params,
                                                     differentiable=self._period_half_differentiable, _prefix="mpd.")
        self.discriminator_layers = self.mrsd.discriminator_layers + self.mpd.discriminator_layers
        self._specs = self.mrsd._specs
        self._init_layers(self.mrsd._layers + self.mpd._layers, device, windows=_window_shapes(self._specs),
                          children=[self.mrsd, self.mpd])

    @property
    def n_discriminators(self):
        return len(self.discriminator_layers)

    def layers_of(self, x):
        if not D._wants_grad(getattr(self, "differentiable", False), x):
            D._no_grad_inputs(x)
        if isinstance(x, torch.Tensor) and x.dim() == 3:          # both checks before any launch
            if x.shape[1] != 1 and not self.flat_channel:
                raise ValueError(f"input with {x.shape[1]} channels and flat_channel=False: the reference fails inside its first "
                                 "conv (the spectrogram of a (B, C, T) input has C channels, the conv expects 1); set flat_channel=True")
            _check_length(x.shape[2], self._specs)
        x = self._prepare(x)
        b, c, t = x.shape
        if c != 1:
            x = x.reshape(b * c, 1, t)
        yield from self.mrsd.layers_of(x, 0, prepared=True)
        yield from self.mpd.layers_of(x, len(self.mrsd.discriminator_layers), prepared=True)


class DifferentiableSpectralDiscriminator(UnivNetSpectralDiscriminator):
    """UnivNetSpectralDiscriminator with a backward to its input (module docstring).  Same arguments and state-dict keys."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        D._check_slopes(self.layers, True)
        _check_grad_layers(self.layers)
        self.differentiable = True


class DifferentiableMultiResolutionSpectralDiscriminator(UnivNetMultiResolutionSpectralDiscriminator):
    """UnivNetMultiResolutionSpectralDiscriminator of DifferentiableSpectralDiscriminator children."""
    _spectral_class = DifferentiableSpectralDiscriminator

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.differentiable = True


class DifferentiableDiscriminator(Discriminator):
    """Discriminator with a backward to its input: differentiable spectral children and a period half built with
    ``differentiable=True``.  With ``flat_channel=True`` a (B, C, T) input gets a (B, C, T) gradient."""
    _spectral_half_class = DifferentiableMultiResolutionSpectralDiscriminator
    _period_half_differentiable = True

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.differentiable = True


def discriminator_for(model_type, discriminator_params, device=None, differentiable=False):
    """codecTrain.py:140-147: the UnivNet discriminator for symAudioDecUniv / UnivNet, the HiFi-GAN one for symAudioDec / HiFiGAN;
    with ``differentiable=True`` the ones with a backward to their input."""
    if model_type in ("symAudioDecUniv", "UnivNet"):
        cls = DifferentiableDiscriminator if differentiable else Discriminator
        return cls(**dict(discriminator_params or {}), device=device)
    if differentiable and model_type in ("symAudioDec", "HiFiGAN"):
        return D.Discriminator(**dict(discriminator_params or {}), device=device, differentiable=True)
    return D.discriminator_for(model_type, discriminator_params, device=device)


def load_discriminator(checkpoint, device=None, differentiable=False):
    """discriminator.load_discriminator for a training checkpoint of any of the four model types."""
    build = functools.partial(discriminator_for, differentiable=True) if differentiable else discriminator_for
    return D.load_discriminator(checkpoint, device, build)
