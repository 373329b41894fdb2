"""GPU: functional.ldl_loss / ldl_artifact_map (dsr_ldl_fwd, dsr_ldl_bwd, csrc/ldl.hip) against tests/ldl_ref.py in float64,
with the same closed form evaluated in fp32 by torch on the CPU as the floor.

The bounds follow the definition's rounding points (include/dsr_hip.h); u = 2^-24, K = k k, rmax = max r of the image.

  r       C roundings of a sum of C terms: |dr| <= rho = C u r.  On the 1/256 grid r and re are exact (rho = 0), so the mask is
          compared with ==; on the noise inputs the device's r and re are the fp32 floor's bit for bit (same operations in the
          same order, no product to contract), so the mask is compared with the floor's, and the reference is checked to have
          no pixel whose float64 and fp32 masks differ.
  mu      r_q + (sum (r - r_q)) / K: |dmu| <= Dmu = (2 K + 5) u rmax + rho_max  (K subtractions and K adds of terms <= rmax,
          a division, an add).  It enters v at second order only, because sum (r - mu) = 0.
  v       sum of K fused d^2 terms and a division: |dv| <= (K + 5) u v + 2 rho_max sqrt(K v / (K - 1))
          + K / (K - 1) (rho_max + Dmu)^2
  V, g    V in double from the fp32 r: |dV| <= 2 rho_max sqrt(V HW / (HW - 1)) + rho_max^2 HW / (HW - 1) = x V;
          g = V^(1/5) rounded once: |dg| <= g relg, relg = u + 0.2 x / (1 - x)
  w       one product: |dw| <= m [ (u + relg) w + g dv (1 + relg) ]
  loss    S_n in double from fp32 factors: |dS| <= sum m (r dv + v rho + rho dv);
          |dloss| <= (sum_n g (1 + relg) dS + relg g S) / M + u loss + 4 |floor - f64|
  dx      sign(x - gt) is exact.  detach_weight: |d dr| <= (dw + 2 u w) / M.  Otherwise, with A = sum over the nt window terms
          of (m r)[q'] (r_s - mu[q']), Am = Adj(m r) >= sum (m r)[q'] and |r_s - mu| <= rmax:
            |dA|  <= [ (nt + 2 + C) u rmax + Dmu + rho_max ] Am          (C only where rho > 0)
            |dT2| <= 2 / (K - 1) [ g (1 + relg) dA + relg g |A| ] + 3 u |T2|
            |dt3| <= |t3| (u + dS / S + 0.8 x / (1 - x)) + |c3| 2 rho_max
            |d dr| <= [ dw + dT2 + dt3 + 4 u (|w| + |T2| + |t3|) ] / M
          The fp32 floor forms r Adj(m r) - Adj(m r mu) AFTER the sums and loses K u rmax Am to cancellation there; its ratio to
          this bound is printed, not asserted.

Worst measured |hip - f64| / bound on the MI355X are recorded in the README."""
import functools
import importlib

import pytest
import torch

import ldl_ref as LR

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
U24 = 2.0 ** -24


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


CASES = [((1, 3, 4, 4), 7), ((2, 3, 7, 5), 7), ((2, 3, 33, 40), 7), ((2, 1, 16, 16), 7), ((3, 3, 64, 96), 7), ((1, 3, 256, 256), 7),
         ((2, 3, 33, 40), 3), ((2, 3, 33, 40), 11), ((1, 3, 12, 12), 3), ((1, 3, 12, 12), 11),
         # past the first turn of every loop over images and tiles (csrc/ldl.hip): N = 5, the four waves of ldl_finalize_kernel take
         # a second image (n += 4); 2 x 2 ragged tiles with N = 6; N = 65, the second lane turn of the loss fold (n += 64);
         # 9 x 9 = 81 tiles, ragged on both axes, the second lane turn of ldl_image_stats (t += 64); then the k = 5 and k = 9
         # instantiations of ldl_tile_kernel and ldl_bwd_kernel
         ((5, 1, 16, 16), 7), ((6, 3, 17, 70), 7), ((65, 1, 8, 8), 3), ((2, 3, 130, 513), 7),
         ((2, 3, 33, 40), 5), ((2, 3, 33, 40), 9), ((1, 3, 12, 12), 5), ((1, 3, 12, 12), 9)]
CASE_IDS = ["x".join(map(str, s)) + f"-k{k}" for s, k in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    seed = 1000 + shape[0] * 7 + shape[2] * 31 + shape[3]
    return LR.grid_inputs(shape, seed) if kind == "grid" else LR.noise_inputs(shape, seed)


@functools.lru_cache(maxsize=None)
def _reference(shape, k, kind):
    """Float64 values, the fp32 floor and the bounds of the module docstring: computed once, read only."""
    x, gt, e = _inputs(shape, kind)
    N, C, H, W = shape
    K, M, hw = k * k, x.numel(), H * W
    x64, gt64, e64 = x.double(), gt.double(), e.double()
    out = {}
    for detach in (False, True):
        xl = x64.clone().requires_grad_(True)
        loss = LR.literal_loss(xl, gt64, e64, k, detach)
        (grad,) = torch.autograd.grad(loss, xl)
        out["loss"], out["grad", detach] = float(loss.detach()), grad
        out["floor_grad", detach] = LR.closed_loss_and_grad(x, gt, e, k, detach)[1].double()
    out["map"] = LR.literal_map(x64, gt64, e64, k)
    out["floor_loss"] = float(LR.closed_loss_and_grad(x, gt, e, k)[0])
    out["floor_map"] = LR.closed_map(x, gt, e, k)
    r, m, mu, v, rbar, V, g, S = LR.closed_parts(x64, gt64, e64, k)
    r32, re32 = LR.residuals(x, gt, e)
    out["mask"], out["mask32"] = m.bool(), ~(r32 < re32)
    out["v"] = v
    # the bounds
    amax = lambda t: t.amax(dim=(1, 2, 3), keepdim=True)
    rmax = amax(r)
    rho_c = 0.0 if kind == "grid" else C * U24
    rho, rho_max = rho_c * r, rho_c * rmax
    dmu = (2 * K + 5) * U24 * rmax + rho_max
    dv = (K + 5) * U24 * v + 2 * rho_max * (K * v / (K - 1)).sqrt() + K / (K - 1) * (rho_max + dmu) ** 2
    xr = (2 * rho_max * (V * hw / (hw - 1)).sqrt() + rho_max ** 2 * hw / (hw - 1)) / V
    assert float(xr.max()) < 1e-3
    relg = U24 + 0.2 * xr / (1 - xr)
    w = g * v * m
    dw = m * ((U24 + relg) * w + g * dv * (1 + relg))
    dS = (m * (r * dv + v * rho + rho * dv)).sum(dim=(1, 2, 3), keepdim=True)
    out["dmap"] = dw
    out["dloss"] = float((g * (1 + relg) * dS + relg * g * S).sum()) / M + U24 * abs(out["loss"])
    Am = LR.box_sum_adjoint(m * r, k)
    nt = LR.box_sum_adjoint(torch.ones_like(r), k)
    A = r * Am - LR.box_sum_adjoint(m * r * mu, k)
    dA = ((nt + 2 + (C if rho_c else 0)) * U24 * rmax + dmu + rho_max) * Am
    T2 = 2 / (K - 1) * g * A
    dT2 = 2 / (K - 1) * (g * (1 + relg) * dA + relg * g * A.abs()) + 3 * U24 * T2.abs()
    c3 = S * 0.2 * V ** -0.8 * 2 / (hw - 1)
    t3 = c3 * (r - rbar)
    dt3 = t3.abs() * (U24 + dS / S + 0.8 * xr / (1 - xr)) + c3.abs() * 2 * rho_max
    out["dgrad", False] = (dw + dT2 + dt3 + 4 * U24 * (w.abs() + T2.abs() + t3.abs())) / M
    out["dgrad", True] = (dw + 2 * U24 * w) / M
    return out


def _run(dev, shape, k, kind, detach):
    F = P("functional")
    x, gt, e = _inputs(shape, kind)
    xd = x.to(dev).requires_grad_(True)
    loss = F.ldl_loss(xd, gt.to(dev), e.to(dev), k, detach)
    loss.backward()
    return loss.detach(), xd.grad


@pytest.mark.parametrize("kind", ["grid", "noise"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_loss_map_and_gradient(dev, case, kind):
    """Loss, map and gradient in both detach_weight modes against float64 within the bounds of the module docstring; the mask
    with == (grid: against float64; noise: against the fp32 floor, whose mask the reference shows to be float64's)."""
    F = P("functional")
    shape, k = case
    ref = _reference(shape, k, kind)
    x, gt, e = _inputs(shape, kind)
    dropped = 1.0 - float(ref["mask"].double().mean())
    assert 0.2 < dropped < 0.8 and 0.2 < 1 - dropped < 0.8, dropped
    assert torch.equal(ref["mask"], ref["mask32"])
    amap = F.ldl_artifact_map(x.to(dev), gt.to(dev), e.to(dev), k)
    assert amap.shape == (shape[0], 1, shape[2], shape[3]) and amap.dtype == torch.float32 and not amap.requires_grad
    amap = amap.double().cpu()
    live = ref["v"] > 0
    assert torch.equal((amap != 0)[live], ref["mask"][live])
    assert float(amap[~ref["mask"]].abs().max()) == 0.0
    mratio = float(((amap - ref["map"]).abs() / ref["dmap"])[ref["mask"] & live].max())
    mfloor = float(((ref["floor_map"].double() - ref["map"]).abs() / ref["dmap"])[ref["mask"] & live].max())
    for detach in (False, True):
        loss, grad = _run(dev, shape, k, kind, detach)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == x.shape
        lerr = abs(float(loss.double().cpu()) - ref["loss"])
        lallowed = ref["dloss"] + 4 * abs(ref["floor_loss"] - ref["loss"])
        want = ref["grad", detach]
        bound = ref["dgrad", detach].expand_as(want)
        g = grad.double().cpu()
        assert float(g[x == gt].abs().sum()) == 0.0                 # sign(0) = 0 (no such element on the noise inputs)
        nz = bound > 0
        gratio = float(((g - want).abs()[nz] / bound[nz]).max())
        assert float((g - want).abs()[~nz].max() if bool((~nz).any()) else 0.0) == 0.0
        fratio = float(((ref["floor_grad", detach] - want).abs()[nz] / bound[nz]).max())
        print(f"ldl {shape} k={k} {kind} detach={detach}: loss {ref['loss']:.6g} |hip - f64| {lerr:.3e} of {lallowed:.3e}; gradient "
              f"worst ratio {gratio:.4f} (fp32 floor {fratio:.4f}); map worst ratio {mratio:.4f} (floor {mfloor:.4f}); dropped {dropped:.2f}")
        assert lerr <= lallowed
        assert gratio <= 1.0
    assert mratio <= 1.0


def test_planted_ties_keep_the_weight_and_equal_elements_get_no_gradient(dev):
    """On the grid: r == re keeps the weight (m = 1), x == gt gives a gradient of exactly 0 in both modes."""
    F = P("functional")
    shape, k = (2, 3, 33, 40), 7
    x, gt, e = _inputs(shape, "grid")
    ref = _reference(shape, k, "grid")
    r, re = LR.residuals(x, gt, e)
    ties = (r == re) & (ref["v"] > 0)
    assert int(ties.sum()) > 10 and int((x == gt).sum()) > 10
    amap = F.ldl_artifact_map(x.to(dev), gt.to(dev), e.to(dev), k).cpu()
    assert bool((amap[ties] > 0).all())
    for detach in (False, True):
        _, grad = _run(dev, shape, k, "grid", detach)
        assert float(grad.cpu()[x == gt].abs().max()) == 0.0 and float(grad.abs().max()) > 0.0


@pytest.mark.parametrize("case", [((2, 3, 33, 40), 7), ((1, 3, 256, 256), 7), ((3, 3, 64, 96), 11), ((65, 1, 8, 8), 3),
                                  ((2, 3, 130, 513), 7)], ids=["33x40", "256x256", "64x96-k11", "65x8x8-k3", "130x513"])
def test_two_runs_give_equal_bits(dev, case):
    F = P("functional")
    shape, k = case
    x, gt, e = _inputs(shape, "noise")
    outs = []
    for _ in range(2):
        loss, grad = _run(dev, shape, k, "noise", False)
        outs.append((loss, grad, F.ldl_artifact_map(x.to(dev), gt.to(dev), e.to(dev), k)))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("detach", [False, True], ids=["through-the-map", "detached"])
def test_backward_scales_by_the_incoming_gradient(dev, detach):
    F = P("functional")
    x, gt, e = _inputs((2, 3, 33, 40), "noise")
    grads = []
    for s in (None, 0.25):
        xd = x.to(dev).requires_grad_(True)
        loss = F.ldl_loss(xd, gt.to(dev), e.to(dev), 7, detach)
        (loss if s is None else F.scale_loss(loss, s)).backward()
        grads.append(xd.grad)
    assert torch.equal(grads[1], grads[0] * 0.25) and float(grads[0].abs().max()) > 0


def test_a_nan_in_pred_reaches_the_loss(dev):
    F = P("functional")
    x, gt, e = _inputs((2, 3, 33, 40), "noise")
    for at in ((0, 1, 5, 7), (1, 2, 32, 39)):
        xn = x.clone()
        xn[at] = float("nan")
        loss = F.ldl_loss(xn.to(dev), gt.to(dev), e.to(dev))
        assert bool(torch.isnan(loss)), at


def test_constant_residual_gives_zero_loss_and_zero_gradient(dev):
    """x = gt + c on the grid: r is constant, V = 0 and every v = 0.  Loss 0 and a finite, zero gradient (torch: NaN).  With a
    second image that is not flat, the flat one still contributes zeros and the other its own values."""
    F = P("functional")
    x, gt, e = _inputs((2, 3, 33, 40), "grid")
    gt = gt * 0.5
    flat = gt + 0.125
    for detach in (False, True):
        xd = flat.to(dev).requires_grad_(True)
        loss = F.ldl_loss(xd, gt.to(dev), e.to(dev), 7, detach)
        loss.backward()
        assert float(loss) == 0.0 and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) == 0.0
    assert float(F.ldl_artifact_map(flat.to(dev), gt.to(dev), e.to(dev)).abs().max()) == 0.0
    mixed = flat.clone()
    mixed[1] = x[1]
    xd = mixed.to(dev).requires_grad_(True)
    loss = F.ldl_loss(xd, gt.to(dev), e.to(dev))
    loss.backward()
    want, gwant = LR.closed_loss_and_grad(mixed.double(), gt.double(), e.double(), 7)
    assert float(want) > 0 and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert float(xd.grad[0].abs().max()) == 0.0 and bool(torch.isfinite(xd.grad).all())
    assert float((xd.grad[1].double().cpu() - gwant[1]).abs().max()) <= 1e-4 * float(gwant[1].abs().max())


def test_bad_arguments_raise(dev):
    F = P("functional")
    x = torch.rand(1, 3, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        F.ldl_loss(x.cpu(), x, x)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        F.ldl_loss(x, x, x.cpu())
    with pytest.raises(TypeError):
        F.ldl_loss(x.half(), x, x)
    with pytest.raises(TypeError):
        F.ldl_artifact_map(x, x.double(), x)
    with pytest.raises(RuntimeError, match="one shape"):
        F.ldl_loss(x, x[:, :2], x)
    with pytest.raises(RuntimeError, match="one shape"):
        F.ldl_loss(x[0], x[0], x[0])
    for k in (1, 4, 13, 7.0, True):
        with pytest.raises(ValueError, match="ksize"):
            F.ldl_loss(x, x, x, ksize=k)
    with pytest.raises(ValueError, match="reflect"):
        F.ldl_loss(x[..., :3], x[..., :3], x[..., :3])
    # a gradient is formed for pred only
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    F.ldl_loss(a, b, torch.rand_like(x)).backward()
    assert a.grad is not None and b.grad is None
