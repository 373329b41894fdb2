"""GPU: utils.imresize.interpolate (torch-convention tables through functional.Imresize / dsr_imresize_f32) against float64
F.interpolate (tests/interpolate_ref.py).

Bound per output, as utils/imresize.py's tests document it for the same kernel:
    (taps_h + taps_w + 4) * 2^-24 * A_h * A_w * max|x|,      A = the largest row sum of |w| of that axis
one rounding per fmaf (taps_h + taps_w of them, each on a partial sum no larger than A_h A_w max|x|); the four extra units
cover the rounding of the float64 weights to fp32 (one unit per pass), the rounding of the float64 reference to fp32 and
second-order terms.  The backward pass has the same form with the transposed tables' list lengths and column sums."""
import importlib

import numpy as np
import pytest
import torch

import interpolate_ref as IR

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
U = 2.0 ** -24
SHAPES = [(2, 3, 17, 23), (1, 3, 40, 33)]
SCALES = [0.15, 0.5, 1.0, 1.5]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _tables(I, h, w, mode, form, s, dev):
    if form == "scale_factor":
        oh, ow = IR.out_size(h, scale_factor=s), IR.out_size(w, scale_factor=s)
        return (oh, ow), I.interpolate_tables(h, oh, mode, s, dev), I.interpolate_tables(w, ow, mode, s, dev)
    oh, ow = IR.out_size(h, scale_factor=s), IR.out_size(w, scale_factor=s) + 1        # a size no scale factor gives
    return (oh, ow), I.interpolate_tables(h, oh, mode, None, dev), I.interpolate_tables(w, ow, mode, None, dev)


@pytest.mark.parametrize("form", ["scale_factor", "size"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("mode", IR.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_within_the_bound(dev, shape, mode, s, form):
    I = P("utils.imresize")
    x = torch.rand(shape, generator=torch.Generator().manual_seed(int(s * 100) + shape[2]))
    (oh, ow), th, tw = _tables(I, shape[2], shape[3], mode, form, s, dev)
    if form == "scale_factor":
        got = I.interpolate(x.to(dev), scale_factor=s, mode=mode)
        want = IR.torch_interpolate(x, scale_factor=s, mode=mode)
    else:
        got = I.interpolate(x.to(dev), size=(oh, ow), mode=mode)
        want = IR.torch_interpolate(x, size=(oh, ow), mode=mode)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (shape[0], shape[1], oh, ow)
    a_h, a_w = IR.row_abs_sum(th.w.cpu().numpy()), IR.row_abs_sum(tw.w.cpu().numpy())
    bound = (th.taps + tw.taps + 4) * U * a_h * a_w * float(x.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    print(f"interpolate {shape} {mode} x{s} {form}: taps {th.taps}+{tw.taps}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_area_half_is_exact_on_dyadic_data(dev):
    """Area at x0.5 on even sizes: every output is the mean of a 2 x 2 block with weights 1/2 per pass; on k / 256 data nothing
    rounds, so the result equals the float64 yardstick."""
    I = P("utils.imresize")
    x = torch.randint(0, 256, (2, 3, 18, 24), generator=torch.Generator().manual_seed(0)).float() / 256.0
    for kw in (dict(scale_factor=0.5), dict(size=(9, 12))):
        got = I.interpolate(x.to(dev), mode="area", **kw)
        assert torch.equal(got.cpu().double(), IR.torch_interpolate(x, mode="area", **kw))


@pytest.mark.parametrize("mode", IR.MODES)
@pytest.mark.parametrize("kw", [dict(scale_factor=0.5), dict(scale_factor=1.5), dict(size=(5, 31))], ids=str)
def test_gradient_against_the_yardsticks_autograd(dev, mode, kw):
    I = P("utils.imresize")
    shape = (1, 2, 17, 23)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(shape, generator=g)
    x64 = x.double().requires_grad_(True)
    want_y = IR.torch_interpolate(x64, mode=mode, **kw)
    dy = torch.randn(want_y.shape, generator=g)
    want_y.backward(dy.double())
    xd = x.to(dev).requires_grad_(True)
    y = I.interpolate(xd, mode=mode, **kw)
    y.backward(dy.to(dev))
    sf = kw.get("scale_factor")
    th = I.interpolate_tables(17, y.shape[2], mode, sf, dev)
    tw = I.interpolate_tables(23, y.shape[3], mode, sf, dev)
    c_h, c_w = IR.row_abs_sum(th.t_w.cpu().numpy()), IR.row_abs_sum(tw.t_w.cpu().numpy())
    bound = (th.q + tw.q + 4) * U * c_h * c_w * float(dy.abs().max())
    err = float((xd.grad.cpu().double() - x64.grad).abs().max())
    print(f"interpolate backward {mode} {kw}: lists {th.q}+{tw.q}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_argument_errors(dev):
    I = P("utils.imresize")
    x = torch.rand(1, 3, 8, 8, device=dev)
    for bad in (lambda: I.interpolate(x), lambda: I.interpolate(x, size=(4, 4), scale_factor=0.5),
                lambda: I.interpolate(x, scale_factor=0.5, mode="nearest"), lambda: I.interpolate(x, scale_factor=0.1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        I.interpolate(x[0], scale_factor=0.5)
