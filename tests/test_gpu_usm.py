"""GPU: utils.degradation.usm_sharp / USMSharp (two dsr_imresize_f32 launches with 51-tap tables, dsr_usm_mask,
dsr_usm_combine) against the float64 yardstick tests/usm_ref.py.

The threshold is a discontinuity, so the inputs are fixed: torch.randint(0, 256, (2, 3, h, w), seed 0) / 255 at 26 x 26 (the
smallest legal size: every pixel reflects on both sides) and at 40 x 29.  In float64 every pixel keeps | |res| 255 - 10 | above
0.030 and 0.0097 grey levels (asserted first); the fp32 blur is within (51 + 51 + 4) 2^-24 max|x| = 106 * 2^-24 of the float64
one (the bound of the resampling kernel, weights summing to 1), i.e. 1.6e-3 grey levels, so the mask must match on EVERY
pixel.  The soft mask is then another blur of the same 0 / 1 values (106 * 2^-24), x - blur and the clamp add a rounding each,
the combination at most six more: (2 * 106 + 8) * 2^-24 on the output, whose factors |sharp - x| and soft are at most 1."""
import importlib

import pytest
import torch

import usm_ref as UR

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
U = 2.0 ** -24
CASES = [pytest.param(26, 26, 0.030, id="26x26"), pytest.param(40, 29, 0.0097, id="40x29")]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _input(h, w):
    return torch.randint(0, 256, (2, 3, h, w), generator=torch.Generator().manual_seed(0)).double() / 255


@pytest.mark.parametrize("h,w,margin", CASES)
def test_usm_sharp_against_the_yardstick(dev, h, w, margin):
    D, Fn, L = P("utils.degradation"), P("functional"), P("_lib")
    x64 = _input(h, w)
    want, mask, got_margin = UR.usm_sharp(x64)
    print(f"usm {h}x{w}: float64 margin {got_margin:.4f} grey levels, masked {float(mask.double().mean()):.3f}")
    assert got_margin > margin > 106 * U * 255
    assert 0.5 < float(mask.double().mean()) < 0.99                                       # both branches run
    x = x64.float().to(dev)
    # the product's own mask, from its own blur: the first two of usm_sharp's four launches
    th, tw = D._usm_tables(h, 50, 0, dev), D._usm_tables(w, 50, 0, dev)
    assert th.taps == tw.taps == 51
    blur, m = torch.empty_like(x), torch.empty_like(x)
    Fn._imresize_launch(x, blur, 6, h, w, h, w, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)
    L.check(L.lib().dsr_usm_mask(Fn._ptr(x), Fn._ptr(blur), 10.0, Fn._ptr(m), x.numel(), Fn._stream()))
    assert float((blur.cpu().double() - UR.blur(x64, UR.gaussian_1d())).abs().max()) <= 106 * U
    assert torch.equal(m.cpu() != 0, mask)                                                # every pixel, none left out
    assert bool(((m == 0) | (m == 1)).all())
    got = D.usm_sharp(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, h, w)
    err = float((got.cpu().double() - want).abs().max())
    print(f"usm {h}x{w}: max error {err:.3e}, bound {(2 * 106 + 8) * U:.3e}")
    assert err <= (2 * 106 + 8) * U
    assert torch.equal(D.USMSharp()(x), got)
    assert float((got.cpu().double() - x64).abs().max()) > 0.05                           # it does sharpen


def test_weight_zero_returns_the_input(dev):
    D = P("utils.degradation")
    x = _input(40, 29).float().to(dev)
    y = D.usm_sharp(x, weight=0.0)
    ulp = torch.maximum(x.abs(), torch.tensor(2.0 ** -126, device=dev)) * 2.0 ** -23
    assert bool(((y - x).abs() <= ulp).all())


def test_too_small_an_image_is_refused(dev):
    D = P("utils.degradation")
    with pytest.raises(ValueError):
        D.usm_sharp(torch.rand(1, 3, 25, 40, device=dev))
    with pytest.raises(ValueError):
        D.usm_sharp(torch.rand(1, 3, 40, 25, device=dev))
    assert tuple(D.usm_sharp(torch.rand(1, 1, 26, 26, device=dev), radius=51, sigma=3.0).shape) == (1, 1, 26, 26)
