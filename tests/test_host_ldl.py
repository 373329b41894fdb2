"""CPU: the yardstick of the LDL artifact-map loss (tests/ldl_ref.py) against torch autograd, the argument checks of
dsr_ldl_fwd / dsr_ldl_bwd, and the loud failures of the Python surface without a GPU.

1. the closed form (what csrc/ldl.hip evaluates) equals autograd of the literal pad / unfold / var / index-assign / l1_loss
   form in float64, loss and gradient, in both detach_weight modes;
2. the reflect fold (box_sum_adjoint) equals autograd of F.pad(mode='reflect') + box sum;
3. the V == 0 rule: a constant residual gives loss 0 and a zero gradient in the closed form (torch's autograd gives NaN);
4. the inputs of tests/test_gpu_ldl.py keep both branches of the mask populated, with ties and zero differences planted;
5. DSR_E_ARG for every bad argument before anything is launched; the workspace query;
6. functional.ldl_loss / ldl_artifact_map and steps.realesrgan_step(ldl_weight=...) raise on bad input."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as TF

import ldl_ref as LR

PKG = "deep-super-resolution_amd"
SHAPES = [(2, 3, 4, 4), (1, 3, 5, 9), (2, 3, 33, 40), (1, 1, 16, 16)]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(shape, generator=g, dtype=torch.float64) for _ in range(3)]


# ----------------------------------------------------------------------------- 1. closed form = autograd of the literal form
@pytest.mark.parametrize("detach", [False, True], ids=["through-the-map", "detached"])
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_equals_autograd_of_the_literal_form(shape, k, detach):
    """The agreement measured when the form was derived was 2e-15 relative on the loss and 6e-15 of the gradient's maximum
    (float64, about 50 roundings deep at k = 7); the test allows 5e-14 of each, a margin of about 8, which is still eleven
    orders of magnitude below any term of the formula going missing."""
    x, gt, e = _rand(shape, 11 + k)
    x.requires_grad_(True)
    want = LR.literal_loss(x, gt, e, k, detach)
    (gwant,) = torch.autograd.grad(want, x)
    with torch.no_grad():
        got, ggot = LR.closed_loss_and_grad(x.detach(), gt, e, k, detach)
        r, re = LR.residuals(x.detach(), gt, e)
    masked = float((r < re).double().mean())
    assert 0.2 < masked < 0.8, masked
    rel = abs(float(got - want)) / abs(float(want))
    grel = float((ggot - gwant).abs().max() / gwant.abs().max())
    print(f"ldl closed form {shape} k={k} detach={detach}: loss rel {rel:.2e}, gradient {grel:.2e} of its maximum; masked {masked:.2f}")
    assert rel < 5e-14 and grel < 5e-14
    assert float((LR.closed_map(x.detach(), gt, e, k) - LR.literal_map(x.detach(), gt, e, k)).abs().max()) < 1e-14


# ----------------------------------------------------------------------------- 2. the reflect fold
FOLD_CASES = [(hw, k) for hw in ((4, 4), (6, 9), (7, 5), (12, 12), (33, 40)) for k in (3, 5, 7, 11) if min(hw) > (k - 1) // 2]


@pytest.mark.parametrize("hw,k", FOLD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_reflect_fold_is_the_adjoint_of_pad_and_box_sum(hw, k):
    p = (k - 1) // 2
    g = torch.Generator().manual_seed(5)
    a = torch.rand((2, 1) + hw, generator=g, dtype=torch.float64, requires_grad=True)
    c = torch.rand((2, 1) + hw, generator=g, dtype=torch.float64)
    box = TF.avg_pool2d(TF.pad(a, [p, p, p, p], mode="reflect"), k, stride=1, divisor_override=1)
    (want,) = torch.autograd.grad((box * c).sum(), a)
    got = LR.box_sum_adjoint(c, k)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert float((LR.box_sum(a.detach(), k) - box.detach()).abs().max()) == 0.0


# ----------------------------------------------------------------------------- 3. V == 0
def test_constant_residual_gives_zero_not_nan():
    g = torch.Generator().manual_seed(3)
    gt = torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64)
    e = torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64)
    x = gt.clone()
    x[0] = torch.round(gt[0] * 256) / 256 + 0.125            # image 0: r constant
    gt[0] = torch.round(gt[0] * 256) / 256
    x[1] = torch.rand((3, 8, 8), generator=g, dtype=torch.float64)
    xl = x.clone().requires_grad_(True)
    lit = LR.literal_loss(xl, gt, e, 7)
    (glit,) = torch.autograd.grad(lit, xl)
    assert not bool(torch.isfinite(glit[0]).all())            # torch: 0 * inf
    loss, grad = LR.closed_loss_and_grad(x, gt, e, 7)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert float(grad[0].abs().max()) == 0.0 and float(grad[1].abs().max()) > 0.0
    assert float(LR.closed_map(x, gt, e, 7)[0].abs().max()) == 0.0
    # image 1 alone: what is left is its own loss and gradient, at image 1's share of M
    l1, g1 = LR.closed_loss_and_grad(x[1:], gt[1:], e[1:], 7)
    assert abs(float(loss) - float(l1) / 2) < 1e-15 and float((grad[1] - g1[0] / 2).abs().max()) < 1e-15


# ----------------------------------------------------------------------------- 4. the GPU tests' inputs
def test_gpu_test_inputs_populate_both_branches():
    for shape in ((1, 3, 4, 4), (2, 3, 33, 40), (2, 1, 16, 16)):
        x, gt, e = LR.grid_inputs(shape, 100)
        r, re = LR.residuals(x.double(), gt.double(), e.double())
        r32, re32 = LR.residuals(x, gt, e)
        assert torch.equal(r32.double(), r) and torch.equal(re32.double(), re)          # exact in fp32
        assert int((r == re).sum()) > 0 and int((x == gt).sum()) > 0
        x, gt, e = LR.noise_inputs(shape, 100)
        assert float((x - gt).std()) == pytest.approx(0.1, rel=0.5)


# ----------------------------------------------------------------------------- 5. the ABI
def test_bad_arguments_return_codes():
    L = P("_lib")
    lib = L.lib()
    E_ARG = -1
    buf = (C.c_float * 1024)()                     # host memory stands in for device pointers: nothing may be launched
    p = (C.cast(buf, C.c_void_p).value + 63) & ~63
    ok = dict(x=p, gt=p + 64, e=p + 128, N=1, C=3, H=8, W=8, k=7, ws=p + 256, loss=p + 512, map=p + 576, up=p + 640, dx=p + 704)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.dsr_ldl_fwd(a["x"], a["gt"], a["e"], a["N"], a["C"], a["H"], a["W"], a["k"], a["ws"], a["loss"], a["map"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.dsr_ldl_bwd(a["x"], a["gt"], a["ws"], a["up"], a["N"], a["C"], a["H"], a["W"], a["k"], 0, a["dx"], None)

    for name in ("x", "gt", "e", "ws", "loss"):
        assert fwd(**{name: None}) == E_ARG and b"null" in lib.dsr_last_error(), name
    for name in ("x", "gt", "ws", "up", "dx"):
        assert bwd(**{name: None}) == E_ARG and b"null" in lib.dsr_last_error(), name
    for call in (fwd, bwd):
        for k in (1, 2, 4, 8, 13, -7):
            assert call(k=k) == E_ARG and b"window" in lib.dsr_last_error(), k
        assert call(H=3) == E_ARG and b"H, W >" in lib.dsr_last_error()              # p = 3: H must exceed it
        assert call(W=3) == E_ARG and b"H, W >" in lib.dsr_last_error()
        assert call(N=0) == E_ARG and call(C=0) == E_ARG
        assert call(N=8, C=4, H=8192, W=8192) == E_ARG and b"2^31" in lib.dsr_last_error()
        assert call(x=ok["x"] + 2) == E_ARG and b"misaligned" in lib.dsr_last_error()
        assert call(ws=ok["ws"] + 4) == E_ARG and b"misaligned" in lib.dsr_last_error()
    assert fwd(map=None, k=4) == E_ARG and b"window" in lib.dsr_last_error()          # the map is optional
    ws = lib.dsr_ldl_workspace
    assert ws(1, 3, 3, 8, 7) == 0 and ws(1, 3, 8, 8, 4) == 0 and ws(0, 3, 8, 8, 7) == 0 and ws(8, 4, 8192, 8192, 7) == 0
    assert ws(1, 3, 4, 4, 7) == 8 * (3 + 5) + 4 * 4 * 16                                # one tile: 3 partials, 5 statistics, 4 planes
    assert ws(2, 3, 33, 40, 7) == 8 * (3 * 2 * 3 + 5 * 2) + 4 * 4 * 2 * 33 * 40         # 16 x 64 tiles: 3 x 1 per image
    assert ws(2, 3, 33, 40, 3) == ws(2, 3, 33, 40, 11)
    assert ws(3, 3, 64, 96, 7) == 8 * (3 * 3 * 8 + 5 * 3) + 4 * 4 * 3 * 64 * 96
    assert lib.dsr_abi_version() == L.ABI_VERSION
    assert "dsr_ldl_workspace" in L._NO_LAUNCH and "dsr_ldl_fwd" not in L._NO_LAUNCH and "dsr_ldl_bwd" not in L._NO_LAUNCH


# ----------------------------------------------------------------------------- 6. the Python surface
def test_python_surface_raises_without_a_gpu():
    F, S = P("functional"), P("steps")
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        F.ldl_loss(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        F.ldl_artifact_map(x, x, x)
    with pytest.raises(ValueError, match="gen_ema"):
        S.realesrgan_step(None, torch.nn.Identity(), None, None, None, x, x, ldl_weight=1.0)
    with pytest.raises(ValueError, match="ldl_weight"):
        S.realesrgan_step(None, torch.nn.Identity(), None, None, None, x, x, ldl_weight=-1.0, gen_ema=torch.nn.Identity())
    with pytest.raises(TypeError):
        S.realesrgan_step(None, torch.nn.Identity(), None, None, None, x, x, 1.0, 0.1, "vanilla", None, None, True, True, False, 1.0)
