"""Cases of tests/golden/univ_disc.npz and an fp64 restatement of the reference's UnivNet discriminator.

The restatement follows the reference line by line in float64 (torch CPU ops on float64 tensors):
  * Discriminator.forward (models/vocoder/UnivNet.py:86-103): (B, C, T) with C != 1 and flat_channel -> (B*C, 1, T);
    mrsd(x) + mpd(x).
  * UnivNetSpectralDiscriminator.forward (models/vocoder/modules/discriminator.py:550-572):
    torchaudio.functional.spectrogram(x, pad=win_length // 2, window, n_fft, hop_length, win_length, power=1.0,
    normalized=False).transpose(-1, -2), which is (torchaudio's documented semantics)
      - ``pad`` zeros on both sides of the signal (constant padding),
      - torch.stft with center=True, pad_mode="reflect": n_fft // 2 samples reflected on both sides,
      - the window zero-padded on both sides to n_fft, centred: (n_fft - win_length) // 2 zeros on the left,
      - frame f = padded[f * hop : f * hop + n_fft] * window, 1 + len(padded) // hop ... frames, one-sided rFFT,
      - magnitude |X| (power = 1, no clamp),
    then the six convs of lines 496-544: NonCausalConv2d pads (k - 1) // 2 on both axes (layers/conv_layer.py:221-224),
    LeakyReLU after all but the last.
  * the period half (HiFiGANMultiPeriodDiscriminator.forward, lines 195-210) as disc_oracle restates it; the window buffer
    comes from the state dict, as register_buffer puts it there (line 488).
  * weight norm folded as torch._weight_norm(v, g, 0); the losses are disc_oracle.losses64.
It is the yardstick both the reference's float32 result and the HIP kernels are measured against.
"""
import numpy as np
import torch
import torch.nn.functional as F

from audiodec_amd import synth
from audiodec_amd import univnet_discriminator as U
from disc_oracle import (DIS_FLAGS, FM_FLAGS, GEN_FLAGS, N_SAMPLE, SEED, _weight64, losses64, sample_index,  # noqa: F401
                         split)

_SPEC = {"channels": 32, "kernel_sizes": [[3, 9], [3, 9], [3, 9], [3, 9], [3, 3], [3, 3]],
         "strides": [[1, 1], [1, 2], [1, 2], [1, 2], [1, 1], [1, 1]], "bias": True, "nonlinear_activation": "LeakyReLU",
         "nonlinear_activation_params": {"negative_slope": 0.2}}
_PERIOD = {"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 32, "downsample_scales": [3, 3, 3, 3, 1],
           "max_downsample_channels": 1024, "bias": True, "nonlinear_activation": "LeakyReLU",
           "nonlinear_activation_params": {"negative_slope": 0.1}, "use_weight_norm": True, "use_spectral_norm": False}

# the shipped discriminator_params (config/autoencoder/symADuniv_vctk_48000_hop300.yaml and the UnivNet vocoder config);
# kernel sizes and strides are lists of lists, as YAML gives them
V3 = dict(fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
          spectral_discriminator_params=_SPEC, periods=[2, 3, 5, 7, 11], period_discriminator_params=_PERIOD)

# reduced widths and resolutions, the reference's own arguments: every feature map fits the fixture.  Windows scaled as the
# shipped ones; the hops are wider (frames are computed independently, and v3 covers the shipped overlap) to keep the maps small
REDUCED = dict(V3, fft_sizes=[512, 1024, 256], hop_sizes=[384, 768, 192], win_lengths=[300, 600, 120],
               spectral_discriminator_params=dict(_SPEC, channels=2),
               period_discriminator_params=dict(_PERIOD, channels=1, max_downsample_channels=4))
# hops and windows scaled exactly as the shipped ones (hop < win_length: neighbouring frames overlap), at one short length;
# two resolutions, so that every map still fits the fixture
OVERLAP = dict(REDUCED, fft_sizes=[512, 256], hop_sizes=[60, 25], win_lengths=[300, 120])
NONORM = dict(REDUCED, spectral_discriminator_params=dict(REDUCED["spectral_discriminator_params"], use_weight_norm=False))
FLAT = dict(REDUCED, flat_channel=True)
# the shipped FFT sizes and windows (they bound the shortest input), wide hops and reduced widths to keep the maps small
SHORT = dict(REDUCED, fft_sizes=[1024, 2048, 512], hop_sizes=[600, 1200, 240], win_lengths=[600, 1200, 240])
PARAMS = {"reduced": REDUCED, "overlap": OVERLAP, "nonorm": NONORM, "flat": FLAT, "short": SHORT, "v3": V3}

# the shortest input the reference accepts with the shipped fft_sizes: the 512-point resolution reflects 256 samples of a
# signal of T + 2 * 120, so T > 16 (period 11 alone would accept T = 11); make_univ_disc_golden.py checks that 16 raises
T_MIN = 17

# case: (params, (B, C, T) of y_hat and of y); the discriminator input is cat([y_hat, y]) = (2B, C, T)
CASES = {
    "t2310": ("reduced", (1, 1, 2310)),       # 2*3*5*7*11: no reflect padding for any period
    "t301": ("reduced", (1, 1, 301)),         # odd length
    "t128": ("reduced", (1, 1, 128)),
    "overlap": ("overlap", (1, 1, 150)),      # the shipped hop / window / FFT proportions
    "nonorm": ("nonorm", (1, 1, 150)),        # plain `weight` keys in the spectral layers
    "stereo": ("flat", (1, 2, 101)),          # C = 2 with flat_channel=True read as (B*C, 1, T)
    "tmin": ("short", (1, 1, T_MIN)),
    "v3": ("v3", (1, 1, 4800)),
}
FULL_CASES = [c for c, (p, _) in CASES.items() if p != "v3"]           # every feature map and spectrogram stored


def state_dict(pname):
    return synth.discriminator_state_dict(PARAMS[pname], SEED)


def inputs(case):
    """(y_hat, y): float32 (B, C, T) each, synthetic audio of distinct streams."""
    _, (b, c, t) = CASES[case]
    rows = [synth.synth_audio(SEED, f"univ_disc/{case}/{i}", t) for i in range(2 * b * c)]
    x = np.stack(rows).reshape(2 * b, c, t).astype(np.float32)
    return x[:b], x[b:]


def spectrogram64(x, window, n_fft, hop, win_length):
    """x (N, T) float64, window (win_length,) float64 -> (N, frames, n_fft // 2 + 1): discriminator.py:557-566."""
    pad = win_length // 2                                                     # line 559
    x = F.pad(x, (pad, pad), "constant", 0.0)                                 # spectrogram(): constant pad on both sides
    x = F.pad(x[:, None], (n_fft // 2, n_fft // 2), "reflect")[:, 0]          # torch.stft center=True, pad_mode="reflect"
    left = (n_fft - win_length) // 2                                          # torch.stft: window padded to n_fft, centred
    w = F.pad(window, (left, n_fft - win_length - left))
    frames = x.unfold(-1, n_fft, hop) * w                                     # (N, frames, n_fft)
    return torch.fft.rfft(frames, dim=-1).abs()                               # one-sided, power = 1; frames already first


def forward64(pname, sd, x, with_spectrograms=False):
    """x (N, C, T) float array -> list (per sub-discriminator) of lists of float64 numpy feature maps
    (and the list of spectrograms, one per resolution, when asked)."""
    p = PARAMS[pname]
    disc = U.Discriminator(**p)
    x = torch.from_numpy(np.asarray(x)).double()
    n, c, t = x.shape
    if c != 1 and p.get("flat_channel", False):
        x = x.reshape(n * c, 1, t)                                            # UnivNet.py:98-100
    outs, specs = [], []
    for sub in disc.mrsd.discriminators:                                      # discriminator.py:635-638
        h = spectrogram64(x[:, 0], sd[sub.window_key].double(), sub.fft_size, sub.hop_size, sub.win_length)
        specs.append(h.numpy())
        h = h[:, None]                                                        # (B, 1, frames, bins)
        o = []
        for L in sub.layers:                                                  # lines 567-570
            w, b = _weight64(sd, L)
            h = F.conv2d(h, w, b, stride=L.stride, padding=L.pad)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h.numpy())
        outs.append(o)
    for period, layers in zip(p["periods"], disc.mpd.discriminator_layers):   # discriminator.py:121-136, as disc_oracle
        h = x
        tt = h.shape[-1]
        if tt % period:
            h = F.pad(h, (0, period - tt % period), "reflect")
        h = h.view(h.shape[0], h.shape[1], -1, period)
        o = []
        for L in layers:
            w, b = _weight64(sd, L)
            h = F.conv2d(h, w, b, stride=(L.stride, 1), padding=(L.pad, 0), groups=L.groups)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h.numpy())
        o[-1] = o[-1].reshape(o[-1].shape[0], -1)
        outs.append(o)
    return (outs, specs) if with_spectrograms else outs


def layer_k(pname):
    """Accumulation length K = C_in/g * taps of every layer, [sub-discriminator][layer] (for error bounds derived from K)."""
    disc = U.Discriminator(**PARAMS[pname])
    return [[L.cin * L.kernel[0] * L.kernel[1] if isinstance(L, U.SpecLayer) else (L.cin // L.groups) * L.kernel for L in ls]
            for ls in disc.discriminator_layers]
