"""Cases of tests/golden/disc.npz and an fp64 restatement of the reference's HiFi-GAN discriminator and GAN losses.

The restatement follows the reference line by line in float64 (torch CPU ops on float64 tensors):
  * Discriminator.forward (models/vocoder/HiFiGAN.py:377-395): (B, C, T) with C != 1 -> (B*C, 1, T); msd(x) + mpd(x).
  * HiFiGANMultiScaleDiscriminator.forward (discriminator.py:432-449): scale s sees x pooled s times by AvgPool1d(4, 2, 2)
    (count_include_pad, so every window divides by 4); each scale runs HiFiGANScaleDiscriminator.forward (lines 323-338):
    conv k15 -> LeakyReLU, grouped strided convs k41 -> LeakyReLU, conv k5 -> LeakyReLU, conv k3 (no activation).
  * HiFiGANMultiPeriodDiscriminator.forward (lines 195-210) over HiFiGANPeriodDiscriminator.forward (lines 111-136): right
    reflect padding to a multiple of the period, view (B, C, T/p, p), (5, 1) convs stride (s, 1) pad (2, 0) -> LeakyReLU,
    output_conv kernel (2, 1) pad (1, 0), flatten(1, -1).
  * weight norm folded as torch._weight_norm(v, g, 0) (the pre-hook of nn.utils.weight_norm).
  * losses (losses/adversarial_loss.py:36-58, 95-132; losses/feat_match_loss.py:35-62): means of (x-1)^2, x^2, |a-b|, x,
    min(x-1, 0), min(-x-1, 0), summed over discriminators / layers and divided as the averaging flags say.
It is the yardstick both the reference's float32 result and the HIP kernels are measured against.
"""
import numpy as np
import torch
import torch.nn.functional as F

from audiodec_amd import discriminator as D
from audiodec_amd import synth

SEED = 1337

# the shipped configs' discriminator_params (config/autoencoder/symAD_vctk_48000_hop300.yaml and every HiFiGAN vocoder)
V1 = dict(
    scales=3, scale_downsample_pooling="AvgPool1d",
    scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
    scale_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [15, 41, 5, 3], "channels": 128,
                                "max_downsample_channels": 1024, "max_groups": 16, "bias": True,
                                "downsample_scales": [4, 4, 4, 4, 1], "nonlinear_activation": "LeakyReLU",
                                "nonlinear_activation_params": {"negative_slope": 0.1}},
    follow_official_norm=True, periods=[2, 3, 5, 7, 11],
    period_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 32,
                                 "downsample_scales": [3, 3, 3, 3, 1], "max_downsample_channels": 1024, "bias": True,
                                 "nonlinear_activation": "LeakyReLU", "nonlinear_activation_params": {"negative_slope": 0.1},
                                 "use_weight_norm": True, "use_spectral_norm": False})

# reduced widths, the reference's own arguments: every feature map fits the fixture
REDUCED = dict(V1, scale_discriminator_params=dict(V1["scale_discriminator_params"], channels=4, max_downsample_channels=32,
                                                   max_groups=4),
               period_discriminator_params=dict(V1["period_discriminator_params"], channels=2, max_downsample_channels=16))
PARAMS = {"reduced": REDUCED, "v1": V1}

# case: (params, (B, C, T) of y_hat and of y); the discriminator input is cat([y_hat, y]) = (2B, C, T)
CASES = {
    "t1203": ("reduced", (1, 1, 1203)),
    "t2310": ("reduced", (1, 1, 2310)),       # 2*3*5*7*11: no reflect padding for any period
    "t11": ("reduced", (1, 1, 11)),           # the shortest input the period 11 reflect padding allows (T > 10)
    "stereo": ("reduced", (1, 2, 401)),       # C = 2 read as (B*C, 1, T)
    "v1": ("v1", (1, 1, 4800)),
}
FULL_CASES = [c for c, (p, _) in CASES.items() if p == "reduced"]     # every feature map stored
N_SAMPLE = 32                                                         # v1: entries sampled per feature map

# loss flag combinations: generator (average_by_discriminators, loss_type), discriminator (same),
# feature matching (average_by_layers, average_by_discriminators, include_final_outputs); entry 0 = the shipped configs'
GEN_FLAGS = [(False, "mse"), (True, "mse"), (False, "hinge"), (True, "hinge")]
DIS_FLAGS = GEN_FLAGS
FM_FLAGS = [(False, False, False), (True, False, False), (False, True, False), (True, True, False),
            (False, False, True), (True, False, True), (False, True, True), (True, True, True)]


def state_dict(pname):
    return synth.discriminator_state_dict(PARAMS[pname], SEED)


def inputs(case):
    """(y_hat, y): float32 (B, C, T) each, synthetic audio of distinct streams."""
    _, (b, c, t) = CASES[case]
    rows = [synth.synth_audio(SEED, f"disc/{case}/{i}", t) for i in range(2 * b * c)]
    x = np.stack(rows).reshape(2 * b, c, t).astype(np.float32)
    return x[:b], x[b:]


def sample_index(n):
    """Fixed flat indices of a feature map with n entries (v1 case)."""
    rng = np.random.Generator(np.random.PCG64([SEED, n]))
    return np.sort(rng.choice(n, size=min(N_SAMPLE, n), replace=False))


def _weight64(sd, L):
    k = L.key
    if f"{k}.weight_g" in sd:
        w = torch._weight_norm(sd[f"{k}.weight_v"].double(), sd[f"{k}.weight_g"].double(), 0)
    else:
        w = sd[f"{k}.weight"].double()
    b = sd[f"{k}.bias"].double() if L.bias else None
    return w, b


def forward64(pname, sd, x):
    """x (N, C, T) float array -> list (per sub-discriminator) of lists of float64 numpy feature maps."""
    p = PARAMS[pname]
    disc = D.Discriminator(**p)
    x = torch.from_numpy(np.asarray(x)).double()
    n, c, t = x.shape
    if c != 1:
        x = x.reshape(n * c, 1, t)                                          # HiFiGAN.py:390-392
    outs = []
    pool = p["scale_downsample_pooling_params"]
    xs = x
    for layers in disc.msd.discriminator_layers:                             # discriminator.py:444-447
        h, o = xs, []
        for L in layers:
            w, b = _weight64(sd, L)
            h = F.conv1d(h, w, b, stride=L.stride, padding=L.pad, groups=L.groups)
            if L.act_slope is not None:
                h = F.leaky_relu(h, L.act_slope)
            o.append(h.numpy())
        outs.append(o)
        xs = F.avg_pool1d(xs, pool["kernel_size"], pool["stride"], pool["padding"])
    for period, layers in zip(p["periods"], disc.mpd.discriminator_layers):  # discriminator.py:121-136
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
    return outs


def split(outs):
    """Feature maps of cat([y_hat, y]) -> (of y_hat, of y): the first half of the rows is y_hat."""
    fake = [[t[:t.shape[0] // 2] for t in o] for o in outs]
    real = [[t[t.shape[0] // 2:] for t in o] for o in outs]
    return fake, real


def gen_adv64(fake, average_by_discriminators, loss_type):
    v = sum(np.mean((o[-1] - 1.0) ** 2) if loss_type == "mse" else -np.mean(o[-1]) for o in fake)
    return v / len(fake) if average_by_discriminators else v


def dis_adv64(fake, real, average_by_discriminators, loss_type):
    if loss_type == "mse":
        r = sum(np.mean((o[-1] - 1.0) ** 2) for o in real)
        f = sum(np.mean(o[-1] ** 2) for o in fake)
    else:
        r = sum(-np.mean(np.minimum(o[-1] - 1.0, 0.0)) for o in real)
        f = sum(-np.mean(np.minimum(-o[-1] - 1.0, 0.0)) for o in fake)
    if average_by_discriminators:
        r, f = r / len(real), f / len(fake)
    return r, f


def feat_match64(fake, real, average_by_layers, average_by_discriminators, include_final_outputs):
    total = 0.0
    for fh, f in zip(fake, real):
        if not include_final_outputs:
            fh, f = fh[:-1], f[:-1]
        v = sum(np.mean(np.abs(a - b)) for a, b in zip(fh, f))
        total += v / len(fh) if average_by_layers else v
    return total / len(fake) if average_by_discriminators else total


def losses64(outs):
    """(gen [len(GEN_FLAGS)], dis [len(DIS_FLAGS), 2], fm [len(FM_FLAGS)]) float64 for the outputs of cat([y_hat, y])."""
    fake, real = split(outs)
    gen = np.array([gen_adv64(fake, *f) for f in GEN_FLAGS])
    dis = np.array([dis_adv64(fake, real, *f) for f in DIS_FLAGS])
    fm = np.array([feat_match64(fake, real, *f) for f in FM_FLAGS])
    return gen, dis, fm
