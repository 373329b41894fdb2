"""MI355X: the Y-channel metrics -- metrics.rgb_to_y, LumaPeakSignalNoiseRatio (PSNR_Y), LumaStructuralSimilarityIndexMeasure
(SSIM_Y) and evaluate_generator(y_channel=True) -- against the float64 yardstick tests/luma_ref.py (fp32 quantisation, float64
luma, crop, MSE, PSNR and SSIM), plus the running state, determinism and HIP-graph capture.

Bars: 1e-4 absolute on PSNR-Y (dB) and SSIM-Y, the bar tests/test_gpu_metrics.py holds the RGB modules to against float64; 1e-6
on rgb_to_y, a few fp32 ulp of a value <= 1."""
import functools
import importlib
import math

import pytest
import torch

import luma_ref

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
BAR = 1e-4
BAR_Y = 1e-6


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


@functools.lru_cache(maxsize=None)
def pair(n, h, w, dtype_name, seed=0):
    """(preds, target) on the CPU in the given dtype: target uniform in [0, 1], preds = target + N(0, 0.05) left unclamped (values
    below 0 and above 1), a few entries of both set to exactly 0.5 (0.5 * 255 = 127.5: the rounding tie)."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * n + h + w)
    t = torch.rand(n, 3, h, w, generator=g)
    p = t + 0.05 * torch.randn(n, 3, h, w, generator=g)
    assert p.min().item() < 0 and p.max().item() > 1
    for k in range(6):
        p[k % n, k % 3, (3 * k + 5) % h, (7 * k + 6) % w] = 0.5
        t[(k + 1) % n, (k + 1) % 3, (5 * k + 6) % h, (3 * k + 7) % w] = 0.5
    dt = DTYPES[dtype_name]
    return p.to(dt), t.to(dt)


@functools.lru_cache(maxsize=None)
def refs(n, h, w, dtype_name, shave, quantize, seed=0):
    """The yardstick's numbers for pair(...): computed once per case, shared, never modified."""
    p, t = pair(n, h, w, dtype_name, seed)
    out = dict(y_p=luma_ref.rgb_to_y(p, shave, quantize), y_t=luma_ref.rgb_to_y(t, shave, quantize),
               psnr=luma_ref.psnr_y(p, t, shave, quantize))
    if min(h, w) - 2 * shave >= 11:
        out["ssim"] = luma_ref.ssim_y(p, t, shave, quantize)
    return out


# ============================================================================= values against the yardstick
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("shave", [0, 1, 4])
@pytest.mark.parametrize("hw,with_ssim", [((23, 37), True), ((32, 32), False)])
def test_luma_metrics_vs_float64(dev, metrics, hw, with_ssim, shave, quantize, dtype_name):
    """23 x 37 with shave 1 is a 21 x 35 region: every row starts at an unaligned element and has an odd length, in all three
    dtypes."""
    h, w = hw
    p, t = pair(2, h, w, dtype_name)
    ref = refs(2, h, w, dtype_name, shave, quantize)
    x, y = p.to(dev), t.to(dev)
    tag = f"{hw} shave {shave} quantize {quantize} {dtype_name}"
    # rgb_to_y
    for img, want in ((x, ref["y_p"]), (y, ref["y_t"])):
        got = metrics.rgb_to_y(img, shave=shave, quantize=quantize)
        assert got.dtype == torch.float32 and got.shape == (2, 1, h - 2 * shave, w - 2 * shave) and not got.requires_grad
        err = (got.double().cpu() - want).abs().max().item()
        print(f"rgb_to_y {tag}: max |HIP - float64| = {err:.3g}")
        assert err <= BAR_Y
    assert torch.equal(metrics.rgb_to_y(x, shave=shave, quantize=quantize), metrics.rgb_to_y(x, shave=shave, quantize=quantize))
    # PSNR-Y
    per = metrics.PSNR_Y(shave=shave, quantize=quantize, reduction="none")(x, y)
    assert per.shape == (2,) and per.dtype == torch.float32 and not per.requires_grad
    err = (per.double().cpu() - ref["psnr"]).abs().max().item()
    print(f"PSNR-Y {tag}: HIP {per.tolist()} float64 {ref['psnr'].tolist()} max err {err:.3g} dB")
    assert err <= BAR
    mean, total = metrics.PSNR_Y(shave, quantize)(x, y), metrics.PSNR_Y(shave, quantize, reduction="sum")(x, y)
    assert mean.shape == () and total.shape == ()
    assert abs(mean.item() - ref["psnr"].mean().item()) <= BAR and abs(total.item() - ref["psnr"].sum().item()) <= 2 * BAR
    assert torch.equal(metrics.PSNR_Y(shave, quantize, reduction="none")(x, y), per)
    assert not metrics.PSNR_Y(shave, quantize)(x.clone().requires_grad_(), y).requires_grad
    if not with_ssim:
        return
    # SSIM-Y
    sper = metrics.SSIM_Y(shave=shave, quantize=quantize, reduction="none")(x, y)
    assert sper.shape == (2,) and sper.dtype == torch.float32 and not sper.requires_grad
    err = (sper.double().cpu() - ref["ssim"]).abs().max().item()
    print(f"SSIM-Y {tag}: HIP {sper.tolist()} float64 {ref['ssim'].tolist()} max err {err:.3g}")
    assert err <= BAR
    smean, stotal = metrics.SSIM_Y(shave, quantize)(x, y), metrics.SSIM_Y(shave, quantize, reduction="sum")(x, y)
    assert abs(smean.item() - ref["ssim"].mean().item()) <= BAR and abs(stotal.item() - ref["ssim"].sum().item()) <= 2 * BAR
    assert torch.equal(metrics.SSIM_Y(shave, quantize, reduction="none")(x, y), sper)
    assert not metrics.SSIM_Y(shave, quantize)(x.clone().requires_grad_(), y).requires_grad
    # the fused path gives the modules' bits
    fp, fs = metrics.luma_psnr_ssim(x, y, shave=shave, quantize=quantize)
    assert torch.equal(fp, per) and torch.equal(fs, sper)
    fp, fs = metrics.luma_psnr_ssim(x, y, shave=shave, quantize=quantize, with_ssim=False)
    assert torch.equal(fp, per) and fs is None


def test_mixed_dtypes_and_strided_inputs(dev, metrics):
    """preds in fp16 against an fp32 target (a half-precision generator scored against the dataset's floats), and a
    non-contiguous view."""
    p, t = pair(2, 23, 37, "fp16")[0], pair(2, 23, 37, "fp32")[1]
    want_p, want_s = luma_ref.psnr_y(p, t, 1, True), luma_ref.ssim_y(p, t, 1, True)
    x, y = p.to(dev), t.to(dev)
    assert (metrics.PSNR_Y(1, reduction="none")(x, y).double().cpu() - want_p).abs().max().item() <= BAR
    assert (metrics.SSIM_Y(1, reduction="none")(x, y).double().cpu() - want_s).abs().max().item() <= BAR
    wide = torch.zeros(2, 3, 23, 40, device=dev)
    wide[..., :37] = y
    assert torch.equal(metrics.PSNR_Y(1, reduction="none")(x, wide[..., :37]), metrics.PSNR_Y(1, reduction="none")(x, y))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_one_green_step_apart(dev, metrics, dtype_name):
    """preds equal the target except one green value one 8-bit step away (code 10 against 11, exact enough in every dtype to
    quantise to those codes), 23 x 37, shave 1: dY^2 = (128.553 / 255^2)^2 at one of 21 x 35 pixels, so PSNR-Y =
    10 log10(21 * 35 * 255^4 / 128.553^2) = 82.74 dB.  A luma subtracted after the conversion (two values near 0.4, each carrying
    ~3e-8 of rounding, against a difference of 2e-3) misses the bar; the channel difference taken first does not."""
    _, t = pair(1, 23, 37, dtype_name)
    t = t.clone()
    t[0, 1, 11, 17] = 10.0 / 255.0
    p = t.clone()
    p[0, 1, 11, 17] = 11.0 / 255.0
    codes = (luma_ref.quantise(p, True) - luma_ref.quantise(t, True)) * 255.0
    assert codes.abs().sum().item() == pytest.approx(1.0, abs=1e-9) and codes[0, 1, 11, 17].item() == pytest.approx(1.0, abs=1e-9)
    closed = 10.0 * math.log10(21 * 35 * 255.0 ** 4 / 128.553 ** 2)
    want = luma_ref.psnr_y(p, t, 1, True)
    assert abs(want.item() - closed) <= 1e-9
    got = metrics.PSNR_Y(shave=1, quantize=True, reduction="none")(p.to(dev), t.to(dev))
    print(f"one green step {dtype_name}: HIP {got.item():.6f} dB, closed form {closed:.6f} dB")
    assert abs(got.item() - closed) <= BAR
    fused, s = metrics.luma_psnr_ssim(p.to(dev), t.to(dev), shave=1, quantize=True)
    assert torch.equal(fused, got)
    assert abs(s.item() - luma_ref.ssim_y(p, t, 1, True).item()) <= BAR
    # the step on the shaved border is not seen
    p2 = t.clone()
    p2[0, 1, 0, 17] = t[0, 1, 0, 17] + (0.25 if t[0, 1, 0, 17] < 0.5 else -0.25)
    assert metrics.PSNR_Y(shave=1)(p2.to(dev), t.to(dev)).item() == math.inf
    assert metrics.PSNR_Y(shave=0)(p2.to(dev), t.to(dev)).item() < 80.0


@pytest.mark.parametrize("quantize", [False, True])
def test_identical_images(dev, metrics, quantize):
    p, _ = pair(2, 23, 37, "fp32")
    x = p.to(dev)
    per = metrics.PSNR_Y(shave=1, quantize=quantize, reduction="none")(x, x.clone())
    assert per.tolist() == [math.inf, math.inf]
    assert metrics.PSNR_Y(shave=1, quantize=quantize)(x, x.clone()).item() == math.inf
    s = metrics.SSIM_Y(shave=1, quantize=quantize, reduction="none")(x, x.clone())
    assert (s.double() - 1.0).abs().max().item() <= 1e-6
    # quantisation makes images that differ by less than half a step identical
    if quantize:
        y = (x.clamp(0, 1) * 255).round() / 255
        assert metrics.PSNR_Y(shave=0)(y + 1e-4, y).item() == math.inf


# ============================================================================= running state
@pytest.mark.parametrize("which", ["psnr", "ssim"])
def test_luma_running_state(dev, metrics, which):
    M = metrics.PSNR_Y if which == "psnr" else metrics.SSIM_Y
    fn = luma_ref.psnr_y if which == "psnr" else luma_ref.ssim_y
    batches = [pair(n, 23, 37, "fp32", seed=n) for n in (1, 3, 2)]
    want_all = torch.cat([fn(p, t, 4, True) for p, t in batches])
    for red in ("elementwise_mean", "sum", "none"):
        m = M(shave=4, reduction=red)
        with pytest.raises(RuntimeError, match="before"):
            m.compute()
        for k, (p, t) in enumerate(batches):
            if k == 1:                                       # forward: the batch's value from a fresh state
                out = m(p.to(dev), t.to(dev))
                w = want_all[1:4]
                want = {"elementwise_mean": w.mean(), "sum": w.sum(), "none": w}[red]
                assert out.shape == want.shape
                assert (out.double().cpu() - want).abs().max().item() <= BAR * (3 if red == "sum" else 1)
            else:
                assert m.update(p.to(dev), t.to(dev)) is None
        got = m.compute()
        want = {"elementwise_mean": want_all.mean(), "sum": want_all.sum(), "none": want_all}[red]
        assert got.shape == want.shape and got.dtype == torch.float32
        assert (got.double().cpu() - want).abs().max().item() <= BAR * (6 if red == "sum" else 1)
        assert m._st.buf.dtype == torch.float64 and m._st.buf.is_cuda
        m.reset()
        with pytest.raises(RuntimeError, match="before"):
            m.compute()
        p, t = batches[2]
        m.update(p.to(dev), t.to(dev))
        w = want_all[4:6]
        want = {"elementwise_mean": w.mean(), "sum": w.sum(), "none": w}[red]
        assert (m.compute().double().cpu() - want).abs().max().item() <= BAR * (2 if red == "sum" else 1)


# ============================================================================= capture
def test_graphed_luma_metrics_replay_bit_identically(dev, metrics):
    """PSNR-Y, SSIM-Y, rgb_to_y and the fused pair, captured with steps.GraphedStep, replay bit for bit what the eager calls give,
    with new values in the input tensors between replays: nothing in them reads the device on the host."""
    steps = P("steps")
    x = torch.empty(2, 3, 23, 37, device=dev, dtype=torch.float16)
    y = torch.empty(2, 3, 23, 37, device=dev)
    psnr_g, ssim_g = metrics.PSNR_Y(shave=1), metrics.SSIM_Y(shave=1, reduction="none")

    def fill(k):
        p, t = pair(2, 23, 37, "fp32", seed=10 + k)
        x.copy_(p.to(dev))
        y.copy_(t.to(dev))

    def step(psnr, ssim, xx, yy):
        fp, fs = metrics.luma_psnr_ssim(xx, yy, shave=1)
        return psnr(xx, yy), ssim(xx, yy), metrics.rgb_to_y(xx, shave=1, quantize=True), fp, fs

    fill(0)
    graphed = steps.GraphedStep(lambda: step(psnr_g, ssim_g, x, y), warmup=2)
    for k in range(1, 4):
        fill(k)
        out_g = [t.clone() for t in graphed()]
        out_e = step(metrics.PSNR_Y(shave=1), metrics.SSIM_Y(shave=1, reduction="none"), x.clone(), y.clone())
        torch.cuda.synchronize()
        for a, b in zip(out_g, out_e):
            assert torch.equal(a, b)
    p, t = pair(2, 23, 37, "fp32", seed=13)
    want = luma_ref.psnr_y(p.half(), t, 1, True)
    assert abs(out_g[0].item() - want.mean().item()) <= BAR and (out_g[3].double().cpu() - want).abs().max().item() <= BAR


# ============================================================================= evaluate_generator(y_channel=True)
@pytest.fixture(scope="module")
def evaluated(dev):
    torch.manual_seed(0)
    gen = P("models.GAN.generator").Generator(4, 1).to(dev)
    g = torch.Generator().manual_seed(7)
    pairs = [(torch.rand(1, 3, 12, 16, generator=g).to(dev), torch.rand(1, 3, 48, 64, generator=g).to(dev), [f"img{i}"])
             for i in range(2)]
    return gen, pairs


def _check_y_keys(res, pairs, srs, shave, with_ssim=True):
    names = [n[0] for _, _, n in pairs]
    assert list(res["psnr_y"]) == names
    want_p = [luma_ref.psnr_y(sr.cpu(), hr.cpu(), shave, True).item() for sr, (_, hr, _) in zip(srs, pairs)]
    for n, wv in zip(names, want_p):
        assert isinstance(res["psnr_y"][n], float) and abs(res["psnr_y"][n] - wv) <= BAR, (n, res["psnr_y"][n], wv)
    assert abs(res["avg_psnr_y"] - sum(want_p) / len(want_p)) <= BAR
    if not with_ssim:
        assert "ssim_y" not in res and "avg_ssim_y" not in res
        return
    assert list(res["ssim_y"]) == names
    want_s = [luma_ref.ssim_y(sr.cpu(), hr.cpu(), shave, True).item() for sr, (_, hr, _) in zip(srs, pairs)]
    for n, wv in zip(names, want_s):
        assert abs(res["ssim_y"][n] - wv) <= BAR, (n, res["ssim_y"][n], wv)
    assert abs(res["avg_ssim_y"] - sum(want_s) / len(want_s)) <= BAR


def test_evaluate_generator_y_channel(dev, evaluated):
    ev, inf = P("evaluate"), P("infer")
    gen, pairs = evaluated
    plain = ev.evaluate_generator(gen, pairs)
    res = ev.evaluate_generator(gen, pairs, y_channel=True)
    assert set(res) == set(plain) | {"avg_psnr_y", "psnr_y", "avg_ssim_y", "ssim_y"}
    for k, v in plain.items():
        assert res[k] == v, k                                # the RGB keys are those of a call without y_channel
    srs = [inf.super_resolve(gen, lr) for lr, _, _ in pairs]
    _check_y_keys(res, pairs, srs, 4)                        # the default shave is the scale factor, 48 // 12
    assert ev.evaluate_generator(gen, pairs, y_channel=True, shave=4) == res
    other = ev.evaluate_generator(gen, pairs, y_channel=True, shave=0, with_ssim=False)
    assert set(other) == {"avg_psnr", "psnr", "avg_psnr_y", "psnr_y"}
    _check_y_keys(other, pairs, srs, 0, with_ssim=False)
    assert other["psnr_y"] != res["psnr_y"]
    tiled = ev.evaluate_generator(gen, pairs, y_channel=True, tile=8)
    _check_y_keys(tiled, pairs, [inf.super_resolve(gen, lr, tile=8) for lr, _, _ in pairs], 4)


def test_evaluate_generator_y_channel_self_ensemble(dev, evaluated):
    ev, inf = P("evaluate"), P("infer")
    gen, pairs = evaluated
    plain = ev.evaluate_generator(gen, pairs, self_ensemble=True)
    res = ev.evaluate_generator(gen, pairs, self_ensemble=True, y_channel=True)
    for k, v in plain.items():
        assert res[k] == v, k
    _check_y_keys(res, pairs, [inf.super_resolve(gen, lr, self_ensemble=True) for lr, _, _ in pairs], 4)


def test_evaluate_generator_y_channel_ema(dev, evaluated):
    ev, inf, O = P("evaluate"), P("infer"), P("optim")
    gen, pairs = evaluated
    ema = O.WeightEMA(gen, decay=0.5)
    saved = [p.detach().clone() for p in gen.parameters()]
    try:
        ema.update()                                         # the first update copies the weights
        with torch.no_grad():
            for p in gen.parameters():
                p.mul_(1.25)
        ema.update()                                         # the average now sits between the two
        own = ev.evaluate_generator(gen, pairs, y_channel=True)
        res = ev.evaluate_generator(gen, pairs, y_channel=True, ema=ema)
        plain = ev.evaluate_generator(gen, pairs, ema=ema)
        for k, v in plain.items():
            assert res[k] == v, k
        with ema.average_parameters():
            srs = [inf.super_resolve(gen, lr) for lr, _, _ in pairs]
        _check_y_keys(res, pairs, srs, 4)                    # the new arguments reach the loop under the averaged weights
        assert res["psnr_y"] != own["psnr_y"]
    finally:
        with torch.no_grad():
            for p, q in zip(gen.parameters(), saved):
                p.copy_(q)
