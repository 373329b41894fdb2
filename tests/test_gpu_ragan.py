"""GPU: functional.relativistic_gan_loss (dsr_rel_gan_loss, csrc/ragan.hip) against tests/ragan_ref.rel_gan_loss in float64,
with the same formula evaluated in fp32 by torch on the CPU as the floor.

The primitive's definition (include/dsr_hip.h) rounds twice on the way to z = x - mu: mu to fp32, then the subtraction.  Both
roundings are at most 2^-24 relative, of mu and of z, so z is off by at most 2^-24 (|mu| + |z|); the bounds below are those of
tests/test_gpu_ganloss.py plus that perturbation carried through l (Lipschitz constant Lip) and l' (curvature c = max |l''|)."""
import functools
import importlib

import pytest
import torch

import ragan_ref as RG

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
E24 = 2.0 ** -24


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _ulp32(t64):
    """One fp32 ulp at each |value| (the spacing of fp32 there; 2^-149 below the normal range)."""
    a = t64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


BIG = (1024 * 1024 + 5, 1024 * 1024 + 7)
SIZES = [pytest.param((1, 1), id="1-1"), pytest.param((2, 3), id="2-3"), pytest.param((128, 192), id="128-192"),
         pytest.param((6720, 6720), id="6720-6720"), pytest.param(BIG, id="past-the-grid-cap")]
SHAPED = {128: (2, 1, 8, 8), 192: (3, 1, 8, 8)}


@functools.lru_cache(maxsize=None)
def _inputs(n, m, off):
    x = RG.logits(n, 1000 + n, off).reshape(SHAPED.get(n, (n,)))
    o = RG.logits(m, 2000 + m, off).reshape(SHAPED.get(m, (m,)))
    return x, o


@functools.lru_cache(maxsize=None)
def _reference(n, m, off, kind, real, is_disc):
    """float64 value and gradients, the fp32 floor, mu and z: computed once, read only."""
    x, o = _inputs(n, m, off)
    x64, o64 = x.double().requires_grad_(True), o.double().requires_grad_(True)
    want = RG.rel_gan_loss(x64, o64, real, kind, is_disc)
    gx, go = torch.autograd.grad(want, (x64, o64))
    floor = RG.rel_gan_loss(x, o, real, kind, is_disc)
    mu = float(o.double().mean())
    z = (x.double() - mu).detach()
    return want.detach(), gx, go, floor.double(), mu, z


@pytest.mark.parametrize("off", [0.0, 50.0], ids=["off0", "off50"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("is_disc", [False, True], ids=["gen", "disc"])
@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
@pytest.mark.parametrize("kind", ["vanilla", "lsgan", "hinge"])
def test_value_and_gradients(dev, kind, real, is_disc, size, off):
    """With Lip = 1 (vanilla, hinge) or 2 max|z - t| (lsgan), c = max |l''| = 1/4, 2, 0 and k the number of elements within 1e-4
    of the hinge's kink (is_disc; their share is at most 1e-3, they are left out of the grad_x check):
        value           |hip - f64| <= 4 |floor - f64| + ulp32(value) + Lip 2^-24 (|mu| + max|z|)
        grad_x[i]       |hip - f64| <= 4 ulp32(g_i) + c 2^-24 (|mu| + |z_i|) / n
        grad_other[j]   all m entries equal bit for bit; |hip - f64| <= 4 ulp32(g) + c 2^-24 mean(|mu| + |z_i|) / m + k / (n m)
    Finite values and gradients at the planted +-30, +-100."""
    F = P("functional")
    n, m = size
    x, o = _inputs(n, m, off)
    want, gx, go, floor, mu, z = _reference(n, m, off, kind, real, is_disc)
    xd, od = x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
    got = F.relativistic_gan_loss(xd, od, real, kind, is_disc)
    got.backward()
    assert got.dtype == torch.float32 and got.dim() == 0 and xd.grad.shape == xd.shape and od.grad.shape == od.shape
    assert bool(torch.isfinite(got)) and bool(torch.isfinite(xd.grad).all()) and bool(torch.isfinite(od.grad).all())
    c = RG.curvature(kind)
    lip = 2 * float((z - (1.0 if real else 0.0)).abs().max()) if kind == "lsgan" else 1.0
    kink = RG.near_kink(z, kind, real, is_disc)
    k = int(kink.sum())
    assert k / n <= 1e-3
    # value
    err = abs(float(got.detach().double().cpu()) - float(want))
    allowed = 4 * abs(float(floor) - float(want)) + float(_ulp32(want.reshape(1))[0]) + lip * E24 * (abs(mu) + float(z.abs().max()))
    # grad_x
    gerr = (xd.grad.double().cpu() - gx).abs()
    gallowed = 4 * _ulp32(gx) + c * E24 * (abs(mu) + z.abs()) / n
    gratio = float((gerr / gallowed)[~kink].max()) if k < n else 0.0
    # grad_other
    flat = od.grad.reshape(-1)
    assert bool((flat.view(torch.int32) == flat.view(torch.int32)[0]).all())
    oerr = abs(float(flat[0].double().cpu()) - float(go.reshape(-1)[0]))
    oallowed = 4 * float(_ulp32(go.reshape(-1)[:1])[0]) + c * E24 * float((abs(mu) + z.abs()).mean()) / m + k / (n * m)
    print(f"rel_gan_loss {kind} real={real} is_disc={is_disc} n={n} m={m} off={off}: value {float(want):.6g} |hip - f64| {err:.3e} of "
          f"{allowed:.3e}; grad_x worst ratio {gratio:.3f}; grad_other {oerr:.3e} of {oallowed:.3e}; near the kink {k}")
    assert err <= allowed
    assert gratio <= 1.0
    assert oerr <= oallowed


@pytest.mark.parametrize("size", [(2, 3), (6720, 6720), BIG], ids=["2-3", "6720-6720", "past-the-grid-cap"])
def test_two_calls_give_equal_bits(dev, size):
    F = P("functional")
    x, o = _inputs(size[0], size[1], 50.0)
    outs = []
    for _ in range(2):
        xd, od = x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
        loss = F.relativistic_gan_loss(xd, od, True, "vanilla", True)
        loss.backward()
        outs.append((loss.detach(), xd.grad, od.grad))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_backward_scales_both_gradients_by_the_incoming_gradient(dev):
    F = P("functional")
    x, o = _inputs(128, 192, 0.0)
    grads = []
    for s in (None, 0.25):
        xd, od = x.to(dev).requires_grad_(True), o.to(dev).requires_grad_(True)
        loss = F.relativistic_gan_loss(xd, od, False, "lsgan")
        (loss if s is None else F.scale_loss(loss, s)).backward()
        grads.append((xd.grad, od.grad))
    assert torch.equal(grads[1][0], grads[0][0] * 0.25) and torch.equal(grads[1][1], grads[0][1] * 0.25)
    assert float(grads[0][0].abs().max()) > 0 and float(grads[0][1].abs().max()) > 0


def test_a_gradient_nobody_needs_is_not_formed(dev):
    """other.requires_grad == False: no other.grad appears, and pred's gradient and the value are what they are with both; the
    same the other way round; under no_grad the value alone."""
    F = P("functional")
    x, o = _inputs(128, 192, 0.0)
    xd, od = x.to(dev).requires_grad_(True), o.to(dev)
    loss = F.relativistic_gan_loss(xd, od, True)
    loss.backward()
    assert od.grad is None and xd.grad is not None
    both_x = x.to(dev).requires_grad_(True)
    both_o = o.to(dev).requires_grad_(True)
    F.relativistic_gan_loss(both_x, both_o, True).backward()
    assert torch.equal(both_x.grad, xd.grad)
    xd2, od2 = x.to(dev), o.to(dev).requires_grad_(True)
    loss2 = F.relativistic_gan_loss(xd2, od2, True)
    loss2.backward()
    assert xd2.grad is None and torch.equal(od2.grad, both_o.grad) and torch.equal(loss2, loss)
    with torch.no_grad():
        plain = F.relativistic_gan_loss(xd, od2, True)
    assert not plain.requires_grad and torch.equal(plain, loss.detach())
    with pytest.raises(ValueError):
        F.relativistic_gan_loss(xd, od, True, kind="wgan")


@pytest.mark.parametrize("n", [1, 6720, BIG[0]])
@pytest.mark.parametrize("is_disc", [False, True], ids=["gen", "disc"])
@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
@pytest.mark.parametrize("kind", ["vanilla", "lsgan", "hinge"])
def test_against_a_zero_mean_it_is_gan_loss(dev, kind, real, is_disc, n):
    """m = 1, other = 0: mu = 0 and z = x exactly, so value and gradient are gan_loss's bit for bit (the same element pass,
    the same partial table, the same fold)."""
    F = P("functional")
    x, _ = _inputs(n, n, 0.0)
    a = x.to(dev).requires_grad_(True)
    b = x.to(dev).requires_grad_(True)
    la = F.relativistic_gan_loss(a, torch.zeros(1, device=dev), real, kind, is_disc)
    lb = F.gan_loss(b, real, kind, is_disc)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach().view(torch.int32), lb.detach().view(torch.int32))
    assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))
