"""GPU: functional.gan_loss (dsr_gan_loss, csrc/pointwise.hip) against tests/unetd_ref.gan_loss in float64, with the same
formula evaluated in fp32 by torch on the CPU as the floor."""
import importlib

import pytest
import torch

import unetd_ref as U

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _logits(shape):
    """N(0, 3^2) logits with the extremes +-30 and +-100 planted (a length-1 tensor: one moderate value)."""
    g = torch.Generator().manual_seed(sum(shape) + len(shape))
    x = torch.randn(shape, generator=g) * 3
    flat = x.reshape(-1)
    if flat.numel() >= 4:
        flat[:4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    return x


def _ulp32(t64):
    """One fp32 ulp at each |value| (the spacing of fp32 there; 2^-149 below the normal range)."""
    a = t64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


SHAPES = [pytest.param((2, 1, 8, 8), id="2x1x8x8"), pytest.param((3, 1, 40, 56), id="3x1x40x56"), pytest.param((1,), id="len1")]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("is_disc", [False, True])
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("kind", ["vanilla", "lsgan", "hinge"])
def test_gan_loss_value_and_gradient(dev, kind, real, is_disc, shape):
    """Value: |hip - f64| <= 4 |floor - f64| + one fp32 ulp of the value, floor = the formula in fp32 on the CPU (4: another,
    fixed summation order and the device's expf / log1pf).  Gradient per element: 4 fp32 ulp against float64.  The extremes
    give finite values and gradients.

    Observed on the MI355X over the 36 cases: the value's deviation stays below 0.2 of what is allowed (largest ratio: lsgan on
    the length-1 tensor, 4.6e-8 of 3.0e-7; vanilla 3 x 1 x 40 x 56: 4.7e-8 of 3.1e-7); the gradient's largest deviation is 2.25 ulp
    (vanilla, 3 x 1 x 40 x 56), 0.50 ulp for lsgan and 0.39 ulp for hinge."""
    F = P("functional")
    x = _logits(shape)
    x64 = x.double().requires_grad_(True)
    want = U.gan_loss(x64, real, kind, is_disc)
    (gwant,) = torch.autograd.grad(want, x64)
    floor = U.gan_loss(x.clone(), real, kind, is_disc)
    xd = x.to(dev).requires_grad_(True)
    got = F.gan_loss(xd, real, kind, is_disc)
    got.backward()
    assert got.dtype == torch.float32 and got.dim() == 0 and xd.grad.shape == xd.shape
    assert bool(torch.isfinite(got)) and bool(torch.isfinite(xd.grad).all())
    dev_err = abs(float(got.detach().double().cpu()) - float(want))
    allowed = 4 * abs(float(floor.double()) - float(want)) + float(_ulp32(want.detach().reshape(1))[0])
    gerr = ((xd.grad.double().cpu() - gwant).abs() / _ulp32(gwant)).max()
    print(f"gan_loss {kind} real={real} is_disc={is_disc} {shape}: value {float(want):.6g}, |hip - f64| {dev_err:.3e}, allowed "
          f"{allowed:.3e}, gradient {float(gerr):.2f} ulp")
    assert dev_err <= allowed
    assert float(gerr) <= 4.0


def test_backward_scales_by_the_incoming_gradient(dev):
    F = P("functional")
    x = _logits((2, 1, 8, 8)).to(dev)
    a = x.clone().requires_grad_(True)
    F.gan_loss(a, True).backward()
    b = x.clone().requires_grad_(True)
    F.scale_loss(F.gan_loss(b, True), 0.25).backward()
    assert torch.equal(b.grad, a.grad * 0.25)
    with pytest.raises(ValueError):
        F.gan_loss(x, True, kind="wgan")
