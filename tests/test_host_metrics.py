"""CPU: the metric modules of metrics.py without a device -- argument checks of the new entry points through the built library,
the constructors' option checks, the inputs they refuse before any launch -- and the float64 references the GPU tests use
(tests/ssim_ref.py against oracle/metrics.py and gradcheck; the coefficient-map form of the gradient that dsr_ssim_bwd_f32
implements, against autograd)."""
import ctypes
import importlib
import math

import pytest
import torch
import torch.nn.functional as TF

import ssim_ref

PKG = "deep-super-resolution_amd"
E_ARG = -1


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def so():
    return P("_build").build()


@pytest.fixture(scope="module")
def metrics():
    return P("metrics")


# ----------------------------------------------------------------------------- the float64 references
def test_ssim_ref_mean_equals_oracle(metrics):
    oracle_metrics = importlib.import_module("oracle.metrics")
    g = torch.Generator().manual_seed(5)
    for shape in [(2, 3, 40, 52), (1, 1, 11, 11), (3, 3, 11, 64)]:
        a = torch.rand(shape, generator=g, dtype=torch.float64)
        b = (a + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
        per = ssim_ref.ssim_per_image(a, b)
        assert per.shape == (shape[0],)
        assert abs(float(per.mean()) - oracle_metrics.ssim(a, b)) <= 1e-12


def test_ssim_ref_gradcheck(metrics):
    g = torch.Generator().manual_seed(6)
    a = torch.rand(1, 2, 13, 15, generator=g, dtype=torch.float64)
    b = (a + 0.2 * torch.randn(1, 2, 13, 15, generator=g, dtype=torch.float64)).clamp(0, 1)
    a.requires_grad_()
    b.requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: ssim_ref.ssim_per_image(x, y), (a, b))


def coefficient_form_grads(a, b, up, data_range=1.0, k1=0.01, k2=0.03):
    """d (sum_n up[n] * per_image[n]) / da, db in float64 the way dsr_ssim_bwd_f32 forms it: the four coefficient maps
    dS/dmu_a, dS/dmu_b, dS/dE[a^2] (= dS/dE[b^2]), dS/dE[ab] at every window position, each correlated with the transposed
    window (conv_transpose2d: zero outside the positions that exist), then
    da = k (W'cmu_a + 2 a W'cE2 + b W'cEab), db = k (W'cmu_b + 2 b W'cE2 + a W'cEab), k = up[n] / (C OH OW)."""
    n, c, h, w = a.shape
    g = ssim_ref.gaussian_window()
    win = (g[:, None] * g[None, :])[None, None].expand(c, 1, 11, 11)
    mu_a, mu_b = TF.conv2d(a, win, groups=c), TF.conv2d(b, win, groups=c)
    e_aa, e_bb, e_ab = TF.conv2d(a * a, win, groups=c), TF.conv2d(b * b, win, groups=c), TF.conv2d(a * b, win, groups=c)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    a1, a2 = 2 * mu_a * mu_b + c1, 2 * (e_ab - mu_a * mu_b) + c2
    b1, b2 = mu_a * mu_a + mu_b * mu_b + c1, (e_aa - mu_a * mu_a) + (e_bb - mu_b * mu_b) + c2
    inv = 1 / (b1 * b2)
    s = a1 * a2 * inv
    d, e = 2 * (a2 - a1) * inv, 2 * s * (1 / b1 - 1 / b2)
    cma, cmb, ce2, ceab = mu_b * d - mu_a * e, mu_a * d - mu_b * e, -s / b2, 2 * a1 * inv

    def tr(m):
        return TF.conv_transpose2d(m, win, groups=c)

    k = (up / (c * (h - 10) * (w - 10))).view(-1, 1, 1, 1)
    da = k * (tr(cma) + 2 * a * tr(ce2) + b * tr(ceab))
    db = k * (tr(cmb) + 2 * b * tr(ce2) + a * tr(ceab))
    return da, db


@pytest.mark.parametrize("shape,noise", [((2, 3, 17, 23), 0.15), ((1, 1, 11, 11), 0.3), ((2, 2, 12, 30), 0.02)])
def test_coefficient_form_equals_autograd(metrics, shape, noise):
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    a = torch.rand(shape, generator=g, dtype=torch.float64)
    b = (a + noise * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    up = torch.linspace(0.5, -1.5, shape[0], dtype=torch.float64)
    x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
    (ssim_ref.ssim_per_image(x, y) * up).sum().backward()
    da, db = coefficient_form_grads(a, b, up)
    for got, ref in ((da, x.grad), (db, y.grad)):
        err = float((got - ref).norm() / ref.norm())
        assert err <= 1e-12, err


# ----------------------------------------------------------------------------- argument checks (no device needed)
def test_new_entry_points_reject_bad_arguments(so, metrics):
    lib = P("_lib").lib()
    one = ctypes.c_void_p(16)                            # a non-null "pointer" that is never dereferenced
    nan, inf = float("nan"), float("inf")

    def fwd(a=one, b=one, n=2, c=3, h=32, w=32, c1=1e-4, c2=9e-4, part=one, per=one, tot=one):
        return lib.dsr_ssim_img_f32(a, b, n, c, h, w, c1, c2, part, per, tot, 1.0, 0, None)

    assert fwd(a=None) == E_ARG and fwd(b=None) == E_ARG and fwd(part=None) == E_ARG
    assert fwd(per=None, tot=None) == E_ARG
    assert fwd(n=0) == E_ARG and fwd(c=0) == E_ARG and fwd(n=-1) == E_ARG
    assert fwd(h=10) == E_ARG and b"11x11" in lib.dsr_last_error()
    assert fwd(w=10) == E_ARG
    for bad in (0.0, -1e-4, nan, inf):
        assert fwd(c1=bad) == E_ARG and fwd(c2=bad) == E_ARG

    def bwd(a=one, b=one, n=2, c=3, h=32, w=32, c1=1e-4, c2=9e-4, g=one, g1=one, g2=None):
        return lib.dsr_ssim_bwd_f32(a, b, n, c, h, w, c1, c2, g, g1, g2, None)

    assert bwd(a=None) == E_ARG and bwd(b=None) == E_ARG and bwd(g=None) == E_ARG
    assert bwd(g1=None, g2=None) == E_ARG and b"neither" in lib.dsr_last_error()
    assert bwd(n=0) == E_ARG and bwd(c=0) == E_ARG
    assert bwd(h=10) == E_ARG and bwd(w=5) == E_ARG
    for bad in (0.0, -1.0, nan, inf):
        assert bwd(c1=bad) == E_ARG and bwd(c2=bad) == E_ARG

    def stats(p=one, t=one, n=2, e=1000, sse=one, keys=one):
        return lib.dsr_psnr_stats_f32(p, t, n, e, sse, keys, None)

    assert stats(p=None) == E_ARG and stats(t=None) == E_ARG and stats(sse=None) == E_ARG and stats(keys=None) == E_ARG
    assert stats(n=0) == E_ARG and stats(e=0) == E_ARG

    def fin(sse=one, keys=one, n=2, e=1000, infer=0, rng=1.0, ls=10 / math.log(10), per=None, val=one, st=None):
        return lib.dsr_psnr_finalize(sse, keys, n, e, infer, rng, ls, per, val, 1.0, st, None)

    assert fin(sse=None) == E_ARG and fin(keys=None) == E_ARG and fin(val=None) == E_ARG
    assert fin(n=0) == E_ARG and fin(e=0) == E_ARG
    for bad in (0.0, -1.0, nan, inf):
        assert fin(rng=bad) == E_ARG and b"data_range" in lib.dsr_last_error()
        assert fin(rng=bad, per=one) == E_ARG
    assert fin(infer=1, per=one) == E_ARG                 # per-image values need a given range
    assert fin(ls=0.0) == E_ARG and fin(ls=nan) == E_ARG

    assert lib.dsr_metric_accumulate(None, 2, one, None) == E_ARG
    assert lib.dsr_metric_accumulate(one, 2, None, None) == E_ARG
    assert lib.dsr_metric_accumulate(one, 0, one, None) == E_ARG

    def comp(st=one, mode=2, infer=0, rng=1.0, out=one):
        return lib.dsr_metric_compute(st, mode, infer, rng, 10 / math.log(10), out, None)

    assert comp(st=None) == E_ARG and comp(out=None) == E_ARG
    assert comp(mode=3) == E_ARG and comp(mode=-1) == E_ARG
    for bad in (0.0, -2.0, nan, inf):
        assert comp(rng=bad) == E_ARG


def test_block_helpers(so, metrics):
    lib = P("_lib").lib()
    assert lib.dsr_ssim_img_blocks(2, 3, 40, 52) == 2 * 3 * 2 * 1    # 30 x 42 positions: 2 row tiles of 16, 1 column tile of 64
    assert lib.dsr_ssim_img_blocks(1, 1, 11, 11) == 1
    assert lib.dsr_ssim_img_blocks(32, 3, 512, 512) == 32 * 3 * 32 * 8
    for args in ((0, 3, 40, 40), (2, 0, 40, 40), (2, 3, 10, 40), (2, 3, 40, 10), (-1, 3, 40, 40)):
        assert lib.dsr_ssim_img_blocks(*args) == 0
    assert lib.dsr_ssim_img_blocks(1 << 20, 64, 2048, 2048) == 0       # 2^31 tiles or more
    assert lib.dsr_psnr_blocks(2, 16384) == 2 and lib.dsr_psnr_blocks(2, 16385) == 4
    assert lib.dsr_psnr_blocks(32, 3 * 512 * 512) == 32 * 48
    for args in ((0, 10), (2, 0), (-1, 10), (2, -5)):
        assert lib.dsr_psnr_blocks(*args) == 0


# ----------------------------------------------------------------------------- the modules' options and inputs
def test_psnr_constructor(metrics):
    M = metrics.PeakSignalNoiseRatio
    m = M()
    assert m.data_range is None and m.dim is None and m.base == 10.0 and m.reduction == "elementwise_mean"
    assert M(data_range=1.0, dim=(1, 2, 3), reduction=None).reduction == "none"
    assert M(data_range=2, dim=[3, 2, 1]).dim == (1, 2, 3)
    assert abs(M(base=math.e).log_scale - 10.0) < 1e-12
    with pytest.raises(ValueError, match="data_range"):
        M(dim=(1, 2, 3))
    with pytest.raises(NotImplementedError, match="dim"):
        M(data_range=1.0, dim=(2, 3))
    with pytest.raises(NotImplementedError, match="dim"):
        M(data_range=1.0, dim=1)
    with pytest.raises(NotImplementedError, match="data_range"):
        M(data_range=(0.0, 1.0))
    for bad in (0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError):
            M(data_range=bad)
    for bad in (0, -10.0, 1.0, float("inf")):
        with pytest.raises(ValueError):
            M(base=bad)
    for bad in ("mean", "max"):
        with pytest.raises(ValueError):
            M(data_range=1.0, dim=(1, 2, 3), reduction=bad)
    with pytest.raises(RuntimeError, match="before"):
        M().compute()


def test_ssim_constructor(metrics):
    M = metrics.StructuralSimilarityIndexMeasure
    m = M()
    assert m.data_range == 1.0 and m.reduction == "elementwise_mean"
    assert abs(m.c1 - 1e-4) < 1e-18 and abs(m.c2 - 9e-4) < 1e-18
    assert M(data_range=255, reduction=None).reduction == "none"
    assert M(sigma=(1.5, 1.5), kernel_size=(11, 11)).data_range == 1.0
    for kw, word in ((dict(gaussian_kernel=False), "gaussian_kernel"), (dict(sigma=1.0), "sigma"), (dict(sigma=(1.5, 2.0)), "sigma"),
                     (dict(kernel_size=7), "kernel_size"), (dict(kernel_size=(11, 9)), "kernel_size"),
                     (dict(return_full_image=True), "return_full_image"),
                     (dict(return_contrast_sensitivity=True), "return_contrast_sensitivity"),
                     (dict(data_range=None), "data_range"), (dict(data_range=(0.0, 1.0)), "data_range")):
        with pytest.raises(NotImplementedError, match=word):
            M(**kw)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M(data_range=bad)
    for kw in (dict(k1=0.0), dict(k2=-0.1), dict(k1=float("nan"))):
        with pytest.raises(ValueError):
            M(**kw)
    for bad in ("mean", "max"):
        with pytest.raises(ValueError):
            M(reduction=bad)
    with pytest.raises(RuntimeError, match="before"):
        M().compute()


@pytest.mark.parametrize("which", ["psnr", "ssim"])
def test_inputs_refused_before_any_launch(metrics, which):
    mod = metrics.PeakSignalNoiseRatio() if which == "psnr" else metrics.StructuralSimilarityIndexMeasure()
    x = torch.rand(2, 3, 16, 16)
    for a, b in ((x, x[:1]), (x[0], x[0]), (x, torch.rand(2, 3, 16, 17)), (torch.rand(2, 3, 10, 16),) * 2,
                 (torch.rand(2, 3, 16, 10),) * 2):
        with pytest.raises(ValueError):
            mod(a, b)
        with pytest.raises(ValueError):
            mod.update(a, b)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mod(x, x)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mod.update(x.half(), x.half())
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        mod(x.clone().requires_grad_(), x)
    with pytest.raises(RuntimeError, match="before"):
        mod.compute()                                    # nothing was added by the refused calls
