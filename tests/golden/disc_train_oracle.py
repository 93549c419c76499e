"""Cases of tests/golden/disc_train.npz and an fp64 restatement of the gradient of the discriminator's own loss,
``real_loss + fake_loss`` of ``DiscriminatorAdversarialLoss`` on ``D(y)`` and ``D(y_hat)`` (trainer/trainerGAN.py:256-294,
trainer/autoencoder.py:117-126), with respect to every parameter of the discriminator, ``weight_g`` and ``weight_v`` included.

The cases and inputs are disc_grad_oracle's.  As there, LeakyReLU has a discontinuous derivative, so the restatement is evaluated
AT GIVEN DECISIONS: ``disc_grad_oracle.features64(..., masks)`` replaces every activation by a multiplication with a constant
mask, once with the masks of the ``y_hat`` pass and once with those of the ``y`` pass, and torch's float64 autograd walks both
passes down to the float64 parameters (the weight-norm composition is ``torch._weight_norm`` in float64, differentiated too).
The mse terms have no decision of their own.
"""
import numpy as np
import torch

import disc_grad_oracle as GO
import disc_oracle as DO

CASES = GO.CASES
REDUCED_CASES = GO.REDUCED_CASES
UPSTREAM = GO.UPSTREAM                              # the gradient is that of UPSTREAM * (real_loss + fake_loss)
# flag set: DiscriminatorAdversarialLoss's (loss_type, average_by_discriminators); "shipped" = the symAD_* configs'
FLAGS = {"shipped": ("mse", False), "mse_avg": ("mse", True)}
N_FULL = 2048                                       # a gradient of more entries than this is stored at N_FULL sampled indices
inputs = GO.inputs                                  # (y_hat, y) of a case


def loss_params(flags):
    kind, avg = FLAGS[flags]
    return {"average_by_discriminators": avg, "loss_type": kind}


def param_index(n, full):
    """The flat indices of a parameter of n entries that the fixture stores: all of them for a reduced-width case up to N_FULL
    entries, else fixed sampled ones (N_FULL for a reduced-width case, disc_oracle.N_SAMPLE for v1)."""
    if full and n <= N_FULL:
        return np.arange(n)
    rng = np.random.Generator(np.random.PCG64([DO.SEED, n]))
    return np.sort(rng.choice(n, size=min(N_FULL if full else DO.N_SAMPLE, n), replace=False))


def masks_of(feats):
    """masks[d][l] = a > 0 of one pass's feature maps (arrays or tensors)."""
    return [[GO._np(a) > 0 for a in o] for o in feats]


def loss64(feats_hat, feats, flags):
    """real_loss + fake_loss of a flag set on torch float64 feature maps (losses/adversarial_loss.py:95-132, mse)."""
    kind, avg = FLAGS[flags]
    assert kind == "mse"
    real = sum(torch.mean((o[-1] - 1.0) ** 2) for o in feats)
    fake = sum(torch.mean(o[-1] ** 2) for o in feats_hat)
    if avg:
        real, fake = real / len(feats), fake / len(feats_hat)
    return real + fake


def grads64(pname, sd, y_hat, y, flags, masks_hat=None, masks=None):
    """{key: d (UPSTREAM * (real_loss + fake_loss)) / d parameter} in float64 at the given decisions of the two passes (default:
    the fp64 forward's own), as numpy arrays of the parameters' shapes."""
    xh, xr = torch.from_numpy(np.asarray(y_hat)).double(), torch.from_numpy(np.asarray(y)).double()
    sd64 = {k: v.detach().double() for k, v in sd.items()}
    if masks_hat is None or masks is None:
        with torch.no_grad():
            masks_hat = masks_of(GO.features64(pname, sd64, xh)) if masks_hat is None else masks_hat
            masks = masks_of(GO.features64(pname, sd64, xr)) if masks is None else masks
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    loss = loss64(GO.features64(pname, leaves, xh, masks_hat), GO.features64(pname, leaves, xr, masks), flags)
    (UPSTREAM * loss).backward()
    return {k: v.grad.numpy() for k, v in leaves.items()}


def plain_grads64(pname, sd, y_hat, y, flags):
    """The same gradients by plain fp64 autograd of disc_oracle's formulas (leaky_relu as torch differentiates it)."""
    xh, xr = torch.from_numpy(np.asarray(y_hat)).double(), torch.from_numpy(np.asarray(y)).double()
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    loss = loss64(GO.features64(pname, leaves, xh), GO.features64(pname, leaves, xr), flags)
    (UPSTREAM * loss).backward()
    return {k: v.grad.numpy() for k, v in leaves.items()}
