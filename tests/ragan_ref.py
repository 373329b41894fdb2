"""Float64 CPU yardstick of the relativistic average GAN loss (functional.relativistic_gan_loss, csrc/ragan.hip) and of
steps.esrgan_step.

The loss is BasicSR's GANLoss on `x - other.mean()` (ESRGANModel.optimize_parameters); no BasicSR package was available, so
parity with BasicSR is unpinned and tests/test_host_ragan.py holds this file to torch's own BCEWithLogits / the published
lsgan and hinge formulas.  The step is restated on the yardsticks the Real-ESRGAN step test uses (rrdb_ref, unetd_ref,
vggfeat_ref, oracle.lowp), in float64 or under their bf16 storage model.  Nothing is imported from the package under test."""
import contextlib

import torch

import rrdb_ref as R
import unetd_ref as U
import vggfeat_ref
from oracle import lowp


def rel_gan_loss(x, other, target_is_real, kind="vanilla", is_disc=False):
    """gan_loss(x - mean(other)) in the dtype of the operands (float64: the yardstick; float32: the floor)."""
    return U.gan_loss(x - other.mean(), target_is_real, kind, is_disc)


def logits(n, seed, off=0.0):
    """The inputs of the primitive's tests: 3 N(0, 1) + off from the given seed, fp32, with the extremes planted for n >= 4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3 + off
    if n >= 4:
        x[:4] = torch.tensor([30.0, -30.0, 100.0, -100.0]) + off
    return x


def curvature(kind):
    """max |l''| of the per-element term: what a perturbation of z does to l'(z)."""
    return {"vanilla": 0.25, "lsgan": 2.0, "hinge": 0.0}[kind]


def near_kink(z64, kind, target_is_real, is_disc, tol=1e-4):
    """Mask of the elements on the hinge's kink (is_disc only): |1 -+ z| < tol in float64."""
    if kind != "hinge" or not is_disc:
        return torch.zeros_like(z64, dtype=torch.bool)
    return (1 + (-z64 if target_is_real else z64)).abs() < tol


def step_reference(gsd, dsd, vsd, lq, gt, dtype, layer_weights, l1_weight, gan_weight, gan_type="vanilla"):
    """steps.esrgan_step in float64 (dtype=None) or under the storage model: the five losses (with their 1/2 inside), the
    generator's gradients, and D's state after its five forwards (weights untouched: the optimiser's step is not restated).
    vsd=None leaves the content term out."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in gsd.items()}
    gt64 = gt.double()
    fake = R.network(leaves, lq, 4, dtype=dtype, fused=False)
    l_pix = (fake - gt64).abs().mean()
    l_percep = torch.zeros((), dtype=torch.float64)
    if vsd is not None:
        ctx = lowp.storage(torch.bfloat16) if dtype is not None else contextlib.nullcontext()
        with ctx:
            l_percep = vggfeat_ref.ref_loss({k: v.double() for k, v in vsd.items()}, fake, gt64, layer_weights, "l1", True, False)
    d = {k: v.double().clone() for k, v in dsd.items()}

    def disc(img):
        y, vec = U.network(d, img, dtype, True, True)
        for name, (u, v) in vec.items():
            d[name + ".weight_u"], d[name + ".weight_v"] = u, v
        return y

    rel = lambda x, o, real, is_disc: rel_gan_loss(x, o, real, gan_type, is_disc)
    with torch.no_grad():
        real_pred = disc(gt64)
    fake_pred = disc(fake)
    l_g_gan = 0.5 * (rel(real_pred, fake_pred, False, False) + rel(fake_pred, real_pred, True, False))
    (l1_weight * l_pix + l_percep + gan_weight * l_g_gan).backward()
    grads = {k: v.grad for k, v in leaves.items()}
    with torch.no_grad():
        fake_pred = disc(fake.detach())
        real_pred = disc(gt64)
        l_d_real = 0.5 * rel(real_pred, fake_pred, True, True)
        fake_pred = disc(fake.detach())
        l_d_fake = 0.5 * rel(fake_pred, real_pred, False, True)
    losses = [float(v.detach()) for v in (l_pix, l_percep, l_g_gan, l_d_real, l_d_fake)]
    return losses, grads, d
