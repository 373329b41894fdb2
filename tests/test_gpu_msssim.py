"""MI355X: metrics.MultiScaleStructuralSimilarityIndexMeasure against the float64 restatement tests/msssim_ref.py -- per-image
values and the [L, N] per-scale values, symmetry and reductions, the running state, the gradient against float64 autograd, the
'relu' clamp, HIP-graph capture -- and steps.gen_msssim_step.

One bar throughout, the rule of test_gpu_metrics.py's gradient test: error <= 4 x max(floor, 1e-6), floor = the error of the same
restatement run in float32 on the CPU against float64.  Inputs are msssim_ref.textured_pair with noise amplitudes in [0.05, 1];
every case asserts on the reference that all per-scale values are above 0.05 (they are above 0.15), so none sits on the clamp."""
import functools
import importlib

import pytest
import torch

import msssim_ref

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
BETAS3 = (0.3, 0.3, 0.4)


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


def amplitudes(n):
    return [0.3] if n == 1 else torch.linspace(0.05, 1.0, n).tolist()


def pair(shape, seed=0):
    """float32-representable (preds, target), so that the device and both CPU restatements see the same numbers."""
    p, t = msssim_ref.textured_pair(shape, amplitudes(shape[0]), 100 + seed)
    return p.float(), t.float()


@functools.lru_cache(maxsize=None)
def raw_reference(shape, levels, seed=0):
    """([L, N] raw per-scale means in float64, the same from the float32 restatement): the expensive part, once per case."""
    p, t = pair(shape, seed)
    r64 = msssim_ref.raw_scales(p.double(), t.double(), levels)
    assert r64.min().item() > 0.05, r64                  # the condition on the inputs: no case sits on the clamp
    return r64, msssim_ref.raw_scales(p, t, levels)


def finish(raw, betas, normalize):
    v = torch.relu(raw) if normalize == "relu" else (raw + 1) / 2 if normalize == "simple" else raw
    return torch.prod(v ** torch.tensor(betas, dtype=raw.dtype).view(-1, 1), dim=0), v


def bar_check(what, got, ref, f32):
    floor = (f32.double() - ref).abs().max().item()
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"{what}: max |HIP - float64| {err:.3g}, floor {floor:.3g}, ratio err/max(floor,1e-6) {err / max(floor, 1e-6):.3g}")
    assert err <= 4 * max(floor, 1e-6), (what, err, floor)


# ============================================================================= values
VALUE_SHAPES = [(2, 3, 192, 192), (2, 3, 176, 209), (1, 1, 256, 181), (4, 3, 512, 512)]


@pytest.mark.parametrize("normalize", ["relu", "simple", None])
@pytest.mark.parametrize("shape", VALUE_SHAPES)
def test_msssim_values_vs_float64(dev, metrics, shape, normalize):
    M = metrics.MultiScaleStructuralSimilarityIndexMeasure
    p, t = pair(shape)
    r64, r32 = raw_reference(shape, 5)
    ref, v_ref = finish(r64, msssim_ref.DEFAULT_BETAS, normalize)
    f32, v_f32 = finish(r32, msssim_ref.DEFAULT_BETAS, normalize)
    m = M(reduction="none", normalize=normalize)
    per = m(p.to(dev), t.to(dev))
    assert per.shape == (shape[0],) and per.dtype == torch.float32 and not per.requires_grad
    assert m.last_scales.shape == (5, shape[0])
    bar_check(f"MS-SSIM {shape} {normalize} per image", per, ref, f32)
    bar_check(f"MS-SSIM {shape} {normalize} per scale", m.last_scales, v_ref, v_f32)


@pytest.mark.parametrize("shape", [(2, 3, 44, 57), (2, 3, 192, 192)])
def test_msssim_three_scales_vs_float64(dev, metrics, shape):
    p, t = pair(shape)
    r64, r32 = raw_reference(shape, 3)
    for normalize in ("relu", "simple", None):
        ref, v_ref = finish(r64, BETAS3, normalize)
        f32, v_f32 = finish(r32, BETAS3, normalize)
        m = metrics.MS_SSIM(reduction="none", betas=BETAS3, normalize=normalize)
        per = m(p.to(dev), t.to(dev))
        bar_check(f"MS-SSIM 3 scales {shape} {normalize} per image", per, ref, f32)
        bar_check(f"MS-SSIM 3 scales {shape} {normalize} per scale", m.last_scales, v_ref, v_f32)


def test_msssim_one_scale_is_ssim(dev, metrics):
    """betas=(1,), normalize=None: the value is plain per-image SSIM (the product form of the same position formula)."""
    p, t = pair((2, 3, 40, 52))
    x, y = p.to(dev), t.to(dev)
    got = metrics.MS_SSIM(reduction="none", betas=(1.0,), normalize=None)(x, y)
    want = metrics.SSIM(reduction="none")(x, y)
    assert (got - want).abs().max().item() <= 1e-6


@pytest.mark.parametrize("shape", [(2, 3, 192, 192), (2, 3, 176, 209)])
def test_msssim_symmetry_and_reductions(dev, metrics, shape):
    M = metrics.MultiScaleStructuralSimilarityIndexMeasure
    p, t = pair(shape)
    x, y = p.to(dev), t.to(dev)
    per = M(reduction="none")(x, y)
    for normalize in ("relu", "simple", None):
        m = M(reduction="none", normalize=normalize)
        assert (m(x, x).double() - 1.0).abs().max().item() <= 1e-6
        assert (m.last_scales.double() - 1.0).abs().max().item() <= 1e-6
    assert (M(reduction="none")(y, x) - per).abs().max().item() <= 1e-6
    s, mean = M(reduction="sum")(x, y), M()(x, y)
    assert s.shape == () and mean.shape == ()
    assert abs(s.item() - per.double().sum().item()) <= 1e-6 * shape[0]
    assert abs(mean.item() - per.double().mean().item()) <= 1e-6
    assert torch.equal(M(reduction=None)(x, y), per) and torch.equal(M()(x, y), mean)      # two runs give the same bits


def test_msssim_half_inputs_computed_in_fp32(dev, metrics):
    shape = (2, 3, 192, 192)
    p, t = pair(shape)
    p16, t16 = p.half(), t.half()
    r64 = msssim_ref.raw_scales(p16.double(), t16.double(), 5)
    r32 = msssim_ref.raw_scales(p16.float(), t16.float(), 5)
    assert r64.min().item() > 0.05
    got = metrics.MS_SSIM(reduction="none")(p16.to(dev), t16.to(dev))
    assert got.dtype == torch.float32
    bar_check("MS-SSIM fp16 inputs", got, finish(r64, msssim_ref.DEFAULT_BETAS, "relu")[0],
              finish(r32, msssim_ref.DEFAULT_BETAS, "relu")[0])
    got = metrics.MS_SSIM(reduction="none")(p.double().to(dev), t.double().to(dev))
    assert got.dtype == torch.float32


# ============================================================================= running state
def test_msssim_running_state(dev, metrics):
    M = metrics.MultiScaleStructuralSimilarityIndexMeasure
    shape = (2, 3, 176, 180)
    batches = [pair(shape, seed=k) for k in range(3)]
    refs, f32s = [], []
    for k in range(3):
        r64, r32 = raw_reference(shape, 5, k)
        refs.append(finish(r64, msssim_ref.DEFAULT_BETAS, "relu")[0])
        f32s.append(finish(r32, msssim_ref.DEFAULT_BETAS, "relu")[0])
    refs, f32s = torch.cat(refs), torch.cat(f32s)
    floor = max((f32s.double() - refs).abs().max().item(), 1e-6)
    for red in ("elementwise_mean", "sum", "none"):
        m = M(reduction=red)
        with pytest.raises(RuntimeError):
            m.compute()
        for k, (a, b) in enumerate(batches):
            out = m(a.to(dev), b.to(dev)) if k == 0 else m.update(a.to(dev), b.to(dev))
            if k == 0:                                       # forward: the batch's value from a fresh state
                want = {"elementwise_mean": refs[:2].mean(), "sum": refs[:2].sum(), "none": refs[:2]}[red]
                assert (out.double().cpu() - want).abs().max().item() <= 4 * floor * (2 if red == "sum" else 1)
            else:
                assert out is None
        got = m.compute()
        want = {"elementwise_mean": refs.mean(), "sum": refs.sum(), "none": refs}[red]
        assert got.shape == want.shape
        err = (got.double().cpu() - want).abs().max().item()
        print(f"MS-SSIM running state {red}: |HIP - float64| {err:.3g}, floor {floor:.3g}")
        assert err <= 4 * floor * (6 if red == "sum" else 1)
        m.reset()
        with pytest.raises(RuntimeError):
            m.compute()
        a, b = batches[1]
        m.update(a.to(dev), b.to(dev))
        if red != "sum":
            want = refs[2:4] if red == "none" else refs[2:4].mean()
            assert (m.compute().double().cpu() - want).abs().max().item() <= 4 * floor


# ============================================================================= gradient
def _ref_grads(p, t, which, up, betas, normalize):
    """Autograd of tests/msssim_ref.py in p's dtype (float64: the reference; float32 on the CPU: the floor).  up: None =
    'elementwise_mean' (upstream through the total), else the per-image weights of sum(per * up)."""
    x, y = p.clone().requires_grad_(which & 1 == 1), t.clone().requires_grad_(which & 2 == 2)
    per, _ = msssim_ref.msssim_per_image(x, y, betas, normalize)
    (per.mean() if up is None else (per * up.to(per.dtype)).sum()).backward()
    return x.grad, y.grad


def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def _grad_case(dev, metrics, shape, which, upstream, betas, normalize, levels):
    p, t = pair(shape)
    raw_reference(shape, levels)                              # asserts the condition on the inputs
    up = None if upstream == "mean" else torch.linspace(1.5, -0.5, shape[0], dtype=torch.float64)
    r1, r2 = _ref_grads(p.double(), t.double(), which, up, betas, normalize)
    f1, f2 = _ref_grads(p, t, which, up, betas, normalize)
    x = p.to(dev).requires_grad_(which & 1 == 1)
    y = t.to(dev).requires_grad_(which & 2 == 2)
    M = metrics.MultiScaleStructuralSimilarityIndexMeasure
    if up is None:
        M(betas=betas, normalize=normalize)(x, y).backward()
    else:
        (M(reduction="none", betas=betas, normalize=normalize)(x, y) * up.float().to(dev)).sum().backward()
    for k, (img, ref, f32) in enumerate(((x, r1, f1), (y, r2, f2))):
        if not which & (1 << k):
            assert img.grad is None
            continue
        assert img.grad.dtype == torch.float32 and img.grad.shape == img.shape
        floor = _rel(f32, ref)
        err = _rel(img.grad.cpu(), ref)
        print(f"MS-SSIM grad {shape} {normalize} L={levels} img{k + 1} of {which} {upstream}: rel L2 {err:.3g}, floor {floor:.3g}, "
              f"ratio err/max(floor,1e-6) {err / max(floor, 1e-6):.3g}")
        assert err <= 4 * max(floor, 1e-6), (err, floor)


@pytest.mark.parametrize("shape", [(2, 3, 192, 192), (2, 3, 176, 209)])
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("upstream", ["weights", "mean"])
def test_msssim_gradient_vs_float64(dev, metrics, shape, which, upstream):
    """Relative L2 error of the HIP gradient against float64 autograd; (176, 209) drops a column at scales 0, 2 and 4, which is
    the un-pool epilogue's edge."""
    _grad_case(dev, metrics, shape, which, upstream, msssim_ref.DEFAULT_BETAS, "relu", 5)


@pytest.mark.parametrize("normalize", ["simple", None])
def test_msssim_gradient_other_modes_and_three_scales(dev, metrics, normalize):
    _grad_case(dev, metrics, (1, 1, 256, 181), 3, "mean", msssim_ref.DEFAULT_BETAS, normalize, 5)
    _grad_case(dev, metrics, (2, 3, 45, 57), 1, "weights", BETAS3, normalize, 3)


def test_msssim_backward_only_where_required(dev, metrics):
    p, t = pair((2, 3, 192, 192))
    x, y = p.to(dev), t.to(dev).requires_grad_()
    loss = 1 - metrics.MS_SSIM()(x, y)
    assert loss.requires_grad
    loss.backward()
    assert x.grad is None and y.grad is not None and y.grad.abs().sum().item() > 0
    xh, yh = p.half().to(dev).requires_grad_(), t.half().to(dev).requires_grad_()
    metrics.MS_SSIM()(xh, yh).backward()
    assert xh.grad.dtype == torch.float16 and yh.grad.dtype == torch.float16
    with torch.no_grad():
        assert not metrics.MS_SSIM()(x, y).requires_grad
    m = metrics.MS_SSIM()
    m.update(x, y)                                           # update never builds a graph
    assert not m.compute().requires_grad


# ============================================================================= the clamp
def test_msssim_relu_clamp_gives_zero_value_and_zero_gradient(dev, metrics):
    """preds = 1 - target on a textured target: the covariance is minus the variance, so the cs means are negative.  Under 'relu'
    the value is exactly 0 and the gradient all zeros and finite (torch autograd gives NaN here: the one deliberate difference).
    The second image of the batch is an ordinary pair and keeps its value and gradient."""
    shape = (2, 3, 192, 192)
    p, t = pair(shape)
    p = p.clone()
    p[0] = 1 - t[0]
    raw = msssim_ref.raw_scales(p.double(), t.double(), 5)
    assert raw[0, 0].item() < -0.5 and raw[:, 1].min().item() > 0.05, raw
    x, y = p.to(dev).requires_grad_(), t.to(dev).requires_grad_()
    m = metrics.MS_SSIM(reduction="none")
    per = m(x, y)
    assert per[0].item() == 0.0 and per[1].item() > 0.1
    assert m.last_scales[0, 0].item() == 0.0
    per.sum().backward()
    for img in (x, y):
        assert torch.isfinite(img.grad).all()
        assert img.grad[0].abs().max().item() == 0.0
        assert img.grad[1].abs().max().item() > 0.0
    ref1, _ = _ref_grads(p[1:].double(), t[1:].double(), 1, torch.ones(1, dtype=torch.float64), msssim_ref.DEFAULT_BETAS, "relu")
    f32, _ = _ref_grads(p[1:], t[1:], 1, torch.ones(1, dtype=torch.float64), msssim_ref.DEFAULT_BETAS, "relu")
    assert _rel(x.grad[1:].cpu(), ref1) <= 4 * max(_rel(f32, ref1), 1e-6)
    assert metrics.MS_SSIM()(x.detach(), y.detach()).item() == 0.5 * per[1].item()


# ============================================================================= capture
def test_graphed_msssim_loss_replays_bit_identically(dev, metrics):
    """1 - MS-SSIM forward + backward captured with steps.GraphedStep replays bit for bit what the eager calls give, with new
    values in the input tensors between replays."""
    steps = P("steps")
    shape = (2, 3, 176, 209)
    x = torch.empty(shape, device=dev, requires_grad=True)
    y = torch.empty(shape, device=dev)
    ms_g = metrics.MS_SSIM()

    def fill(k):
        a, b = pair(shape, seed=10 + k)
        with torch.no_grad():
            x.copy_(a.to(dev))
            y.copy_(b.to(dev))

    def step(ms, xx, yy):
        loss = 1 - ms(xx, yy)
        (gx,) = torch.autograd.grad(loss, [xx])
        return loss.detach(), gx, ms.last_scales

    fill(0)
    graphed = steps.GraphedStep(lambda: step(ms_g, x, y), warmup=2)
    for k in range(1, 4):
        fill(k)
        out_g = [t.clone() for t in graphed()]
        xe = x.detach().clone().requires_grad_()
        out_e = step(metrics.MS_SSIM(), xe, y.clone())
        torch.cuda.synchronize()
        for p, q in zip(out_g, out_e):
            assert torch.equal(p, q)
    assert out_g[1].abs().sum().item() > 0


# ============================================================================= the step recipe
ALPHA = 0.84


def _make_step(dev, lr_rate=1e-4, teacher=False):
    """A small generator (x4, 2 blocks), 48 x 48 -> 192 x 192, and a target near its first output, so that the pair is as well
    conditioned as the value tests' inputs: the generator's first output plus uniform noise of amplitude 0.2, or (`teacher`) the
    output of the same generator with every conv weight perturbed by 0.2 of that weight's standard deviation -- a target the
    trained generator can reach, which noise is not."""
    from oracle import filler, gan
    Gm, optim, steps, metrics = P("models.GAN.generator"), P("optim"), P("steps"), P("metrics")
    sd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    lr = filler.tensor("in:ms_lr", (2, 3, 48, 48), 0.5, 0.5).to(dev)
    g = Gm.Generator(4, 2)
    g.load_state_dict(sd)
    g.to(dev).train()
    with torch.no_grad():
        first = g(lr).float()
    g.load_state_dict(sd)                                    # the BatchNorm running statistics as before that forward
    if teacher:
        gen = torch.Generator().manual_seed(11)
        sd_t = {k: v + 0.2 * v.std() * torch.randn(v.shape, generator=gen) if v.dim() == 4 and k.endswith("weight") else v.clone()
                for k, v in sd.items()}
        t = Gm.Generator(4, 2)
        t.load_state_dict(sd_t)
        t.to(dev).train()
        with torch.no_grad():
            hr = t(lr).float().clamp(-1, 1)
    else:
        noise = torch.rand(first.shape, generator=torch.Generator().manual_seed(7)) - 0.5
        hr = (first + 0.2 * noise.to(dev)).clamp(-1, 1)
    opt = optim.FusedAdam(g.parameters(), lr=lr_rate)
    ms = metrics.MS_SSIM(data_range=2.0)
    return g, ms, hr, (lambda: steps.gen_msssim_step(g, opt, ms, lr, hr, ALPHA))


def test_gen_msssim_step_loss_vs_float64(dev):
    _, ms, hr, step = _make_step(dev)
    dis, l1, fake = step()
    assert dis.shape == () and l1.shape == () and fake.shape == hr.shape
    f, h = fake.float().cpu(), hr.float().cpu()

    def composed(a, b):
        per, v = msssim_ref.msssim_per_image(a, b, data_range=2.0)
        return ALPHA * (1 - per.mean()) + (1 - ALPHA) * (a - b).abs().mean(), v

    ref, v = composed(f.double(), h.double())
    assert v.min().item() > 0.05, v
    f32, _ = composed(f, h)
    got = ALPHA * dis.double().cpu() + (1 - ALPHA) * l1.double().cpu()
    bar_check("gen_msssim_step loss", got, ref, f32)
    assert torch.equal(1 - ms(fake, hr), dis)


def test_gen_msssim_step_graphed_is_reproducible_and_equals_eager(dev):
    """Two GraphedSteps built from the same state and replayed twice leave bit for bit the same losses and parameters, and
    what four eager steps leave (two warm-up steps + two replays)."""
    steps = P("steps")
    runs = []
    for _ in range(2):
        g, _, _, step = _make_step(dev)
        graphed = steps.GraphedStep(step, warmup=2)
        for _ in range(2):
            out = graphed()
        torch.cuda.synchronize()
        runs.append(([o.clone() for o in out], {k: v.clone() for k, v in g.state_dict().items()}))
    g_e, _, _, step_e = _make_step(dev)
    for _ in range(4):
        out_e = step_e()
    runs.append((list(out_e), g_e.state_dict()))
    for out, sd in runs[1:]:
        for p, q in zip(runs[0][0], out):
            assert torch.equal(p, q)
        for k, v in runs[0][1].items():
            assert torch.equal(v, sd[k]), k
    assert runs[0][0][0].item() > 0


def test_gen_msssim_step_lowers_the_loss(dev):
    """20 Adam steps on one fixed batch lower 1 - MS-SSIM (last < first; monotonic decrease is not required).  The target is the
    teacher's output: with the noise target of the tests above the generator already sits at the minimum of the expected loss
    (the noise is independent of anything it can compute), and Adam's fixed-size first steps can only move its output away."""
    _, ms, _, step = _make_step(dev, teacher=True)
    vals = []
    for k in range(20):
        vals.append(float(step()[0]))
        if k == 0:
            assert ms.last_scales.min().item() > 0.05, ms.last_scales      # the pair does not sit on the clamp
    print("1 - MS-SSIM over 20 steps", [round(v, 5) for v in vals])
    assert vals[-1] < vals[0], vals
