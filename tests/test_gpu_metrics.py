"""MI355X: metrics.PeakSignalNoiseRatio and metrics.StructuralSimilarityIndexMeasure against float64 restatements -- SSIM per
image against tests/ssim_ref.py, PSNR against its formula in float64, the SSIM gradient against float64 autograd of
tests/ssim_ref.py with a floor measured in the test -- plus the running state, determinism and HIP-graph capture."""
import importlib
import math

import pytest
import torch

import ssim_ref
from oracle import filler

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


@pytest.fixture(scope="module")
def metrics():
    return P("metrics")


def pair(shape, noise, tag=""):
    """A noise-perturbed, clamped pair in [0, 1], as in test_ssim_kernel_vs_oracle."""
    a = filler.tensor("msim:a" + tag + str(shape), shape, 0.5, 0.5)
    b = (a + filler.tensor("msim:n" + tag + str(shape), shape, noise)).clamp(0, 1)
    return a, b


# ============================================================================= SSIM values
SSIM_SHAPES = [(2, 3, 40, 52), (1, 1, 11, 11), (1, 3, 97, 33), (3, 3, 11, 64), (2, 3, 512, 512)]


@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_per_image_vs_float64(dev, metrics, shape):
    M = metrics.StructuralSimilarityIndexMeasure
    a, b = pair(shape, 0.15)
    ref = ssim_ref.ssim_per_image(a.double(), b.double())
    x, y = a.to(dev), b.to(dev)
    per = M(reduction="none")(x, y)
    assert per.shape == (shape[0],) and per.dtype == torch.float32 and not per.requires_grad
    err = (per.double().cpu() - ref).abs().max().item()
    print(f"SSIM {shape}: max |HIP - float64| per image = {err:.3g}")
    assert err <= 1e-4, (per, ref)
    # identical inputs give 1, swapped inputs the same value
    assert (M(reduction="none")(x, x).double() - 1.0).abs().max().item() <= 1e-6
    assert (M(reduction="none")(y, x) - per).abs().max().item() <= 1e-6
    # 'sum' and 'elementwise_mean' against 'none'
    s, m = M(reduction="sum")(x, y), M()(x, y)
    assert s.shape == () and m.shape == ()
    assert abs(s.item() - per.double().sum().item()) <= 1e-6 * shape[0]
    assert abs(m.item() - per.double().mean().item()) <= 1e-6
    # two runs give the same bits
    assert torch.equal(M(reduction="none")(x, y), per) and torch.equal(M()(x, y), m)


def test_ssim_running_state(dev, metrics):
    M = metrics.StructuralSimilarityIndexMeasure
    batches = [pair((2, 3, 40, 52), 0.1 * (k + 1), tag=str(k)) for k in range(3)]
    refs = torch.cat([ssim_ref.ssim_per_image(a.double(), b.double()) for a, b in batches])
    for red in ("elementwise_mean", "sum", "none"):
        m = M(reduction=red)
        with pytest.raises(RuntimeError):
            m.compute()
        for k, (a, b) in enumerate(batches):
            out = m(a.to(dev), b.to(dev)) if k == 0 else m.update(a.to(dev), b.to(dev))
            if k == 0:                                       # forward: the batch's value from a fresh state
                want = {"elementwise_mean": refs[:2].mean(), "sum": refs[:2].sum(), "none": refs[:2]}[red]
                assert (out.double().cpu() - want).abs().max().item() <= 1e-4
        got = m.compute()
        want = {"elementwise_mean": refs.mean(), "sum": refs.sum(), "none": refs}[red]
        assert got.shape == want.shape
        assert (got.double().cpu() - want).abs().max().item() <= 1e-4 * (6 if red == "sum" else 1)
        m.reset()
        with pytest.raises(RuntimeError):
            m.compute()
        a, b = batches[1]
        m.update(a.to(dev), b.to(dev))
        if red != "sum":
            assert (m.compute().double().cpu() - (refs[2:4] if red == "none" else refs[2:4].mean())).abs().max().item() <= 1e-4


def test_ssim_half_inputs_computed_in_fp32(dev, metrics):
    a, b = pair((2, 3, 40, 52), 0.15)
    a16, b16 = a.half(), b.half()
    ref = ssim_ref.ssim_per_image(a16.double(), b16.double())
    got = metrics.StructuralSimilarityIndexMeasure(reduction="none")(a16.to(dev), b16.to(dev))
    assert got.dtype == torch.float32 and (got.double().cpu() - ref).abs().max().item() <= 1e-4


# ============================================================================= PSNR values
def psnr64(p, t, data_range=None, base=10.0):
    p, t = p.double(), t.double()
    mse = ((p - t) ** 2).mean()
    r = data_range if data_range is not None else max(t.max().item(), 0.0) - min(t.min().item(), 0.0)
    return (10.0 / math.log(base)) * (2 * math.log(r) - math.log(mse.item()))


@pytest.mark.parametrize("shape", [(2, 3, 40, 52), (3, 3, 13, 17), (2, 3, 512, 512), (1, 1, 11, 11)])
def test_psnr_vs_float64(dev, metrics, shape):
    M = metrics.PeakSignalNoiseRatio
    a, b = pair(shape, 0.1)
    p = a + filler.tensor("psnr:q" + str(shape), shape, 0.05)          # preds outside [0, 1] too
    t = b * 1.3 - 0.1                                                   # a target range that moves the inferred range
    x, y = p.to(dev), t.to(dev)
    for kw in ({}, dict(data_range=1.0), dict(data_range=2.5, base=2.0)):
        got = M(**kw)(x, y)
        assert got.shape == () and not got.requires_grad
        ref = psnr64(p, t, kw.get("data_range"), kw.get("base", 10.0))
        print(f"PSNR {shape} {kw}: HIP {got.item():.6f} float64 {ref:.6f}")
        assert abs(got.item() - ref) <= 1e-4
    refs = torch.tensor([psnr64(p[i:i + 1], t[i:i + 1], 1.0) for i in range(shape[0])], dtype=torch.float64)
    for red in ("elementwise_mean", "sum", "none", None):
        got = M(data_range=1.0, dim=(1, 2, 3), reduction=red)(x, y)
        want = {"elementwise_mean": refs.mean(), "sum": refs.sum(), "none": refs, None: refs}[red]
        assert got.shape == want.shape
        assert (got.double().cpu() - want).abs().max().item() <= 1e-4 * (shape[0] if red == "sum" else 1)
    # half inputs are computed in fp32; requires_grad inputs give a result without a graph
    got = M()(x.half(), y.half())
    assert abs(got.item() - psnr64(p.half(), t.half())) <= 1e-4
    assert not M()(x.clone().requires_grad_(), y).requires_grad
    assert torch.equal(M()(x, y), M()(x, y))


def test_psnr_running_state(dev, metrics):
    """update()s whose targets move the running min / max (from 0: [0.2, 0.8] leaves (0, 0.8), then -0.3, then 1.7), compute,
    reset."""
    M = metrics.PeakSignalNoiseRatio
    shape = (2, 3, 24, 20)
    ts = [filler.tensor("run:t0", shape, 0.3, 0.5), filler.tensor("run:t1", shape, 0.4, 0.1),
          filler.tensor("run:t2", shape, 0.8, 0.9)]
    ps = [t + filler.tensor(f"run:n{k}", shape, 0.07) for k, t in enumerate(ts)]
    lo = min(0.0, min(t.min().item() for t in ts))
    hi = max(0.0, max(t.max().item() for t in ts))
    sse = sum(((p.double() - t.double()) ** 2).sum().item() for p, t in zip(ps, ts))
    cnt = sum(t.numel() for t in ts)
    for kw in ({}, dict(data_range=1.0)):
        m = M(**kw)
        with pytest.raises(RuntimeError):
            m.compute()
        for k, (p, t) in enumerate(zip(ps, ts)):
            if k == 1:
                out = m(p.to(dev), t.to(dev))                 # forward: the batch's value from a fresh state
                assert abs(out.item() - psnr64(p, t, kw.get("data_range"))) <= 1e-4
            else:
                m.update(p.to(dev), t.to(dev))
            r = kw.get("data_range", None)
            if r is None:
                r = max(0.0, max(x.max().item() for x in ts[:k + 1])) - min(0.0, min(x.min().item() for x in ts[:k + 1]))
            s = sum(((x.double() - y.double()) ** 2).sum().item() for x, y in zip(ps[:k + 1], ts[:k + 1]))
            n = sum(y.numel() for y in ts[:k + 1])
            want = 10 * math.log10(r * r / (s / n))
            got = m.compute().item()
            print(f"PSNR running {kw} after {k + 1} batches: HIP {got:.6f} float64 {want:.6f}")
            assert abs(got - want) <= 1e-4
        want = 10 * math.log10((kw.get("data_range") or (hi - lo)) ** 2 / (sse / cnt))
        assert abs(m.compute().item() - want) <= 1e-4
        m.reset()
        with pytest.raises(RuntimeError):
            m.compute()
        m.update(ps[2].to(dev), ts[2].to(dev))
        assert abs(m.compute().item() - psnr64(ps[2], ts[2], kw.get("data_range"))) <= 1e-4
    # per image: the mean / sum / concatenation over every image of every update
    refs = torch.tensor([psnr64(p[i:i + 1], t[i:i + 1], 1.0) for p, t in zip(ps, ts) for i in range(2)], dtype=torch.float64)
    for red in ("elementwise_mean", "sum", "none"):
        m = M(data_range=1.0, dim=(1, 2, 3), reduction=red)
        for p, t in zip(ps, ts):
            m.update(p.to(dev), t.to(dev))
        want = {"elementwise_mean": refs.mean(), "sum": refs.sum(), "none": refs}[red]
        got = m.compute()
        assert got.shape == want.shape
        assert (got.double().cpu() - want).abs().max().item() <= 1e-4 * (6 if red == "sum" else 1)


# ============================================================================= SSIM gradient
GRAD_CASES = [((2, 3, 64, 80), 0.15), ((2, 3, 64, 80), 0.02), ((1, 3, 128, 96), 0.3), ((4, 1, 11, 11), 0.15)]


def _ref_grads(a, b, which, up):
    """Autograd of tests/ssim_ref.py in a's dtype (float64: the reference; float32 on the CPU: the floor).  up: None =
    'elementwise_mean', else the per-image weights of sum(per * up)."""
    x, y = a.clone().requires_grad_(which & 1 == 1), b.clone().requires_grad_(which & 2 == 2)
    per = ssim_ref.ssim_per_image(x, y)
    (per.mean() if up is None else (per * up.to(per.dtype)).sum()).backward()
    return x.grad, y.grad


def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("shape,noise", GRAD_CASES)
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("upstream", ["weights", "mean"])
def test_ssim_gradient_vs_float64(dev, metrics, shape, noise, which, upstream):
    """Relative L2 error of the HIP gradient against float64 autograd, at most 4 x max(floor, 1e-6); floor = the same error of
    float32 CPU autograd of the restatement."""
    a, b = pair(shape, noise, tag="g")
    up = None if upstream == "mean" else torch.linspace(1.5, -0.5, shape[0], dtype=torch.float64)
    r1, r2 = _ref_grads(a.double(), b.double(), which, up)
    f1, f2 = _ref_grads(a.float(), b.float(), which, up)
    x = a.to(dev).requires_grad_(which & 1 == 1)
    y = b.to(dev).requires_grad_(which & 2 == 2)
    if up is None:
        metrics.StructuralSimilarityIndexMeasure()(x, y).backward()
    else:
        (metrics.StructuralSimilarityIndexMeasure(reduction="none")(x, y) * up.float().to(dev)).sum().backward()
    for k, (img, ref, f32) in enumerate(((x, r1, f1), (y, r2, f2))):
        if not which & (1 << k):
            assert img.grad is None
            continue
        assert img.grad.dtype == torch.float32 and img.grad.shape == img.shape
        floor = _rel(f32, ref)
        err = _rel(img.grad.cpu(), ref)
        bar = 4 * max(floor, 1e-6)
        print(f"SSIM grad {shape} noise {noise} img{k + 1} of {which} {upstream}: rel L2 {err:.3g}, floor {floor:.3g}, "
              f"ratio err/max(floor,1e-6) {err / max(floor, 1e-6):.3g}")
        assert err <= bar, (err, floor)


def test_ssim_backward_only_where_required(dev, metrics):
    """Only img2 requires a gradient: img1.grad stays None; the gradient comes back in each input's dtype."""
    a, b = pair((2, 3, 40, 52), 0.15)
    x, y = a.to(dev), b.to(dev).requires_grad_()
    loss = 1 - metrics.StructuralSimilarityIndexMeasure()(x, y)
    assert loss.requires_grad
    loss.backward()
    assert x.grad is None and y.grad is not None
    _, r2 = _ref_grads(a.double(), b.double(), 2, None)
    assert _rel(-y.grad.cpu(), r2) <= 1e-4
    xh, yh = a.half().to(dev).requires_grad_(), b.half().to(dev).requires_grad_()
    metrics.StructuralSimilarityIndexMeasure()(xh, yh).backward()
    assert xh.grad.dtype == torch.float16 and yh.grad.dtype == torch.float16
    with torch.no_grad():
        assert not metrics.StructuralSimilarityIndexMeasure()(x, y).requires_grad


# ============================================================================= capture
def test_graphed_ssim_loss_and_psnr_replay_bit_identically(dev, metrics):
    """1 - SSIM forward + backward and the PSNR forward, captured with steps.GraphedStep, replay bit for bit what the eager calls
    give, with new values in the input tensors between replays."""
    steps = P("steps")
    shape = (2, 3, 64, 80)
    x = torch.empty(shape, device=dev, requires_grad=True)
    y = torch.empty(shape, device=dev)
    ssim_g, psnr_g = metrics.StructuralSimilarityIndexMeasure(), metrics.PeakSignalNoiseRatio()

    def fill(k):
        a, b = pair(shape, 0.1 + 0.05 * k, tag=f"cap{k}")
        with torch.no_grad():
            x.copy_(a.to(dev))
            y.copy_(b.to(dev))

    def step(ssim, psnr, xx, yy):
        loss = 1 - ssim(xx, yy)
        (gx,) = torch.autograd.grad(loss, [xx])
        return loss.detach(), gx, psnr(xx.detach(), yy)

    fill(0)
    graphed = steps.GraphedStep(lambda: step(ssim_g, psnr_g, x, y), warmup=2)
    for k in range(1, 4):
        fill(k)
        out_g = [t.clone() for t in graphed()]
        xe = x.detach().clone().requires_grad_()
        out_e = step(metrics.StructuralSimilarityIndexMeasure(), metrics.PeakSignalNoiseRatio(), xe, y.clone())
        torch.cuda.synchronize()
        for p, q in zip(out_g, out_e):
            assert torch.equal(p, q)
    assert out_g[1].abs().sum().item() > 0
