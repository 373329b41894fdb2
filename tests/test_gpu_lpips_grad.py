"""GPU: the LPIPS backward on the HIP path (lpips.LPIPS as a training loss; csrc/lpips.hip dsr_lpips_distance_bwd,
dsr_maxpool3s2_bwd, dsr_lpips_stem_prep_bwd and the five input-gradient convolutions) -- each kernel against float64 on
16-bit-representable inputs, then the image gradient against float64 autograd of tests/lpips_ref.py, the launches, and the
perceptual fine-tuning step (steps.gen_lpips_step), eager and replayed from a HIP graph."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as TF

import lpips_ref
import parity_util
from test_host_lpips_grad import distance_grads, maxpool3s2_bwd_gather, quantised

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}        # half an ulp, relative: one rounding to the storage type


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    L = P("_lib")
    return L.F16 if dtype == torch.float16 else L.BF16


def _round_once(x64, dtype):
    """float64 -> storage type with ONE rounding.  (torch casts double to a 16-bit type through float; the values here are sums
    of a few 16-bit numbers of similar magnitude, exact in float, so the first step rounds nothing.)"""
    f = x64.float()
    assert torch.equal(f.double(), x64)
    return f.to(dtype)


# ============================================================================= kernels
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cp", [64, 192])
@pytest.mark.parametrize("with_addend", [False, True])
def test_maxpool3s2_bwd_vs_float64(dev, dtype, cp, with_addend):
    """Equal to the float64 gather-form result (== autograd of max_pool2d, test_host_lpips_grad.py) times the ReLU mask, plus
    the addend, rounded once.  Inputs on a k/8 grid (ties at positive values in most windows, asserted), dy and addend on a
    k/32 grid: every sum is exact in fp32 and needs more bits than bf16 keeps, so the one rounding is exercised."""
    L = P("_lib")
    g = torch.Generator().manual_seed(cp + int(with_addend))
    for h, w in [(7, 7), (8, 8), (9, 12), (15, 6), (3, 3), (31, 30)]:
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        x = quantised((2, cp, h, w), 2, g)
        win = TF.unfold(x[:, :8].reshape(-1, 1, h, w), 3, stride=2)
        mx = win.max(dim=1, keepdim=True).values
        assert float((((win == mx).sum(dim=1) > 1) & (mx[:, 0] > 0)).double().mean()) > 0.5
        dy = torch.randint(-64, 65, (2, cp, oh, ow), generator=g).double() / 32
        add = torch.randint(-64, 65, (2, cp, h, w), generator=g).double() / 32 if with_addend else None
        for relu_mask in (1, 0):
            ref = maxpool3s2_bwd_gather(x, dy)
            if relu_mask:
                ref = ref * (x > 0)
            if add is not None:
                ref = ref + add
            nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
            xd, dyd, addd = nhwc(x), nhwc(dy), (None if add is None else nhwc(add))
            assert torch.equal(xd.cpu().double(), x.permute(0, 2, 3, 1)) and torch.equal(dyd.cpu().double(), dy.permute(0, 2, 3, 1))
            dx = torch.full((2, h, w, cp), float("nan"), dtype=dtype, device=dev)
            L.check(L.lib().dsr_maxpool3s2_bwd(_code(dtype), _ptr(xd), _ptr(dyd), _ptr(addd), _ptr(dx), 2, h, w, cp, relu_mask, _st()))
            torch.cuda.synchronize()
            want = _round_once(ref.permute(0, 2, 3, 1).contiguous(), dtype)
            assert torch.equal(dx.cpu(), want), (h, w, relu_mask, float((dx.cpu().double() - want.double()).abs().max()))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("normalize", [False, True])
def test_stem_prep_bwd_vs_autograd(dev, dtype, normalize):
    """dsr_lpips_stem_prep_bwd == autograd of scale_input + pad + space_to_depth (float64) of the same 16-bit gradient, divided
    by the loss scale.  The kernel multiplies by one fp32 constant per channel: two fp32 roundings (the constant, the product)
    + the store = 3 * 2^-24 relative."""
    L, m = P("_lib"), P("lpips")
    g = torch.Generator().manual_seed(31)
    scale = 1024.0
    for n, h, w in [(2, 33, 35), (1, 64, 64), (2, 97, 131), (1, 31, 31)]:
        oh, ow = m.LPIPS().tap_sizes(h, w)[0]
        bh, bw = oh + 2, ow + 2
        up = torch.randn(n, bh, bw, 64, generator=g).to(dtype)
        x = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64).requires_grad_()
        lpips_ref.space_to_depth(TF.pad(lpips_ref.scale_input(x, normalize), (2, 2, 2, 2)), bh, bw).backward(up.double() / scale)
        out = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=dev)
        L.check(L.lib().dsr_lpips_stem_prep_bwd(_code(dtype), _ptr(up.to(dev)), n, h, w, int(normalize), scale, _ptr(out), _st()))
        torch.cuda.synchronize()
        err = (out.cpu().double() - x.grad).abs()
        assert bool((err <= 3 * 2.0 ** -24 * x.grad.abs()).all()), (n, h, w, float((err / x.grad.abs().clamp_min(1e-30)).max()))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("halves", [1, 2, 3])
def test_distance_bwd_vs_float64(dev, dtype, halves):
    """All five taps in one launch, ReLU-like features with zeros, one all-zero pixel per image side, a different upstream
    gradient per image.  Per element: |got - ref| <= 2 * (one rounding of the storage type) * |ref| + the fp32 accumulation
    error of the two channel reductions, C * 2^-24 relative to the absolute sums they accumulate (|f|^2 under the root, and
    <|u|, |n|> in the projection term), + half an fp16 subnormal step where fp16 is the storage type."""
    L = P("_lib")
    g = torch.Generator().manual_seed(41 + halves)
    n, scale = 3, 256.0
    shapes = [(19, 17, 64), (9, 8, 192), (4, 4, 384), (4, 4, 256), (4, 4, 256)]
    up = torch.tensor([0.7, 0.05, 1.9])
    feats, lins = [], []
    for h, w, c in shapes:
        f = TF.relu(torch.randn(2 * n, h, w, c, generator=g)).to(dtype)
        f[0, 1, 1] = 0                                    # all-zero feature vector in image 1 ...
        f[n + 1, 2, 2] = 0                                # ... and in image 2
        f[2, 0, 0] = 0
        f[n + 2, 0, 0] = 0                                # ... and in both at one pixel
        feats.append(f)
        lins.append(torch.rand(c, generator=g))
    fd = [f.to(dev) for f in feats]
    lw = [w.to(dev) for w in lins]
    out = [torch.full((n * (2 if halves == 3 else 1),) + f.shape[1:], float("nan"), dtype=dtype, device=dev) for f in feats]
    hw = (ctypes.c_int * 5)(*[h * w for h, w, _ in shapes])
    cp = (ctypes.c_int * 5)(*[c for _, _, c in shapes])
    tab = lambda ts: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])
    d1 = tab(out) if halves & 1 else None
    d2 = tab([o[n:] for o in out] if halves == 3 else out) if halves & 2 else None
    L.check(L.lib().dsr_lpips_distance_bwd(_code(dtype), 5, tab(fd), tab(lw), hw, cp, cp, n, _ptr(up.to(dev)), scale, d1, d2, _st()))
    torch.cuda.synchronize()
    for k, (h, w, c) in enumerate(shapes):
        f1, f2 = (feats[k][:n].double().permute(0, 3, 1, 2), feats[k][n:].double().permute(0, 3, 1, 2))
        r1, r2 = distance_grads(f1, f2, lins[k], up.double() * scale)
        refs, srcs = [], []
        if halves & 1:
            refs.append(r1 * (f1 > 0)), srcs.append((f1, f2))
        if halves & 2:
            refs.append(r2 * (f2 > 0)), srcs.append((f2, f1))
        got = out[k].cpu().double().permute(0, 3, 1, 2)
        for i, (ref, (fa, fb)) in enumerate(zip(refs, srcs)):
            sa = torch.sqrt(1e-8 + (fa * fa).sum(1, keepdim=True))
            sb = torch.sqrt(1e-8 + (fb * fb).sum(1, keepdim=True))
            na, nb = fa / sa, fb / sb
            u = (2 * lins[k].double().view(1, -1, 1, 1) * (na - nb) * (up.double() * scale).view(-1, 1, 1, 1) / (h * w)).abs()
            acc = c * 2.0 ** -24 * (4 * u + 4 * na * (u * na).sum(1, keepdim=True)) / sa
            tol = 2 * EPS[dtype] * ref.abs() + acc + (2.0 ** -25 if dtype == torch.float16 else 0.0)
            part = got[i * n:(i + 1) * n]
            assert bool(torch.isfinite(part).all())
            bad = (part - ref).abs() > tol
            assert not bool(bad.any()), (k, i, int(bad.sum()), float(((part - ref).abs() / tol).max()))
            assert bool((part[fa == 0] == 0).all())       # the ReLU mask


def _dgrad_shapes(h, w):
    m = P("lpips")
    s = m.LPIPS().tap_sizes(h, w)
    return [(0, s[0][0] + 2, s[0][1] + 2), (1, s[1][0], s[1][1]), (2, s[2][0], s[2][1]), (3, s[2][0], s[2][1]), (4, s[2][0], s[2][1])]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_five_dgrad_shapes_vs_conv_transpose(dev, dtype):
    """dsr_conv_dgrad on the trunk's five layers (the stem as 3x3 pad 0 64 -> 64; 5x5 pad 2 64 -> 192; 3x3 192 -> 384,
    384 -> 256, 256 -> 256) against float64 conv_transpose2d of the same 16-bit dy and 16-bit weights.  Bound per element: one
    rounding of the stored result (doubled) + fp32 accumulation, K * 2^-24 of the sum of absolute products (K = Cout * taps).
    dsr_conv_dgrad_masked on the same launch equals the plain result times (x_act > 0) bit for bit."""
    L, m = P("_lib"), P("lpips")
    lib = L.lib()
    mod = m.LPIPS(dtype=dtype).to(dev)
    wd = mod._weights_dgrad(dev)
    g = torch.Generator().manual_seed(51)
    for (n, h, w) in [(2, 64, 64), (1, 97, 131)]:
        for k, ih, iw in _dgrad_shapes(h, w):
            _, cout, cin, ks, _, pad = m.ALEX_CONVS[k]
            cin, ks, pad = (64, 3, 0) if k == 0 else (cin, ks, pad)
            oh, ow = ih + 2 * pad - ks + 1, iw + 2 * pad - ks + 1
            dy = torch.randn(n, oh, ow, cout, generator=g).to(dtype)
            w16 = getattr(mod, f"w{k + 1}").cpu().to(dtype).double()
            dyc = dy.double().permute(0, 3, 1, 2)
            ref = TF.conv_transpose2d(dyc, w16, padding=pad).permute(0, 2, 3, 1)
            mag = TF.conv_transpose2d(dyc.abs(), w16.abs(), padding=pad).permute(0, 2, 3, 1)
            assert ref.shape == (n, ih, iw, cin)
            d = L.ConvDesc(_code(dtype), n, ih, iw, cin, cout, ks, ks, 1, pad, L.PAD_ZERO)
            dx = torch.full((n, ih, iw, cin), float("nan"), dtype=dtype, device=dev)
            dyd = dy.to(dev)
            L.check(lib.dsr_conv_dgrad(ctypes.byref(d), _ptr(dyd), _ptr(wd[k]), _ptr(dx), None, 0, _st()))
            torch.cuda.synchronize()
            tol = 2 * EPS[dtype] * ref.abs() + cout * ks * ks * 2.0 ** -24 * mag + (2.0 ** -25 if dtype == torch.float16 else 0.0)
            err = (dx.cpu().double() - ref).abs()
            assert bool((err <= tol).all()), (n, h, w, k, float((err / tol).max()))
            assert lib.dsr_conv_dgrad_masked_supported(ctypes.byref(d)) == 1
            xa = TF.relu(torch.randn(n, ih, iw, cin, generator=g)).to(dtype).to(dev)
            dm = torch.full_like(dx, float("nan"))
            L.check(lib.dsr_conv_dgrad_masked(ctypes.byref(d), _ptr(dyd), _ptr(wd[k]), _ptr(xa), L.ACT_RELU, 0.0, _ptr(dm), _st()))
            torch.cuda.synchronize()
            assert torch.equal(dm, torch.where(xa > 0, dx, torch.zeros_like(dx))), (n, h, w, k)


# ============================================================================= the module
def _pair(shape, seed, normalize=False, close=True):
    g = torch.Generator().manual_seed(seed)
    lo = 0.0 if normalize else -1.0
    a = torch.rand(shape, generator=g) * (1 - lo) + lo
    if close:
        b = (a + 0.1 * (1 - lo) * torch.randn(shape, generator=g)).clamp(lo, 1.0)
    else:
        b = torch.rand(shape, generator=g) * (1 - lo) + lo
    return a, b


def _weights():
    m = P("lpips")
    return m.load_net_state(m._standin_alex_state()), m.load_lin_state(m._standin_lin_state())


def _ref_grads(a, b, reduction, normalize, storage=None, scale=1.0):
    """float64 autograd of lpips_ref.lpips_per_image w.r.t. both images.  storage: a 16-bit type -> the storage-model run
    (oracle/lowp.py: every conv's input, weight and output, and the gradients through them, rounded to it), with the static
    loss scale the product uses, so that the fp16 floor is not one of flushed gradients."""
    from oracle import lowp
    net, lins = _weights()
    x, y = a.double().requires_grad_(), b.double().requires_grad_()

    def run():
        per = lpips_ref.lpips_per_image(x, y, net, lins, normalize)
        ((per.mean() if reduction == "mean" else per.sum()) * scale).backward()

    if storage is None:
        run()
    else:
        with lowp.storage(storage):
            run()
    return x.grad / scale, y.grad / scale


def test_backward_exists_and_reaches_only_what_requires_it(dev):
    """The test that fails without the feature: LPIPS()(x.requires_grad_(), y).backward()."""
    m = P("lpips")
    a, b = _pair((2, 3, 64, 72), 1)
    mod = m.LPIPS()
    for need_a, need_b in ((True, False), (False, True), (True, True)):
        x, y = a.to(dev).requires_grad_(need_a), b.to(dev).requires_grad_(need_b)
        out = mod(x, y)
        assert out.requires_grad and out.grad_fn is not None and out.shape == ()
        out.backward()
        for t, need in ((x, need_a), (y, need_b)):
            if need:
                assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32
                assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
            else:
                assert t.grad is None
    # no graph without a reason for one; update() never builds one
    with torch.no_grad():
        assert not mod(a.to(dev).requires_grad_(), b.to(dev)).requires_grad
    assert not mod(a.to(dev), b.to(dev)).requires_grad
    mod.update(a.to(dev).requires_grad_(), b.to(dev))
    assert not mod.compute().requires_grad and not mod.sum_scores.requires_grad
    per = mod.per_image(a.to(dev).requires_grad_(), b.to(dev))
    assert per.requires_grad and per.shape == (2,)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_image_gradient_vs_float64(dev, dtype, normalize, reduction):
    """Both image gradients against float64 autograd of the restatement, non-square size not divisible by 4, close and
    unrelated pairs, unchunked and chunked (one pair per trunk pass).  Bar: the rule of tests/parity_util.py against the
    storage-model floor, 1 - cos <= 1.5 * (1 - cos_floor) + 0.01 and norm ratio within 3 %.  Measured values: DESIGN.md.
    The chunked run must also sit within 2^-8 of the largest gradient element of the unchunked one: the trunk passes differ
    only in the tile a convolution picks for the batch, i.e. in accumulation order, which can move each of the chain's six
    stored 16-bit gradients by an ulp (2^-11 of its magnitude for fp16, 2^-8 for bf16, where the bar is 2^-5 likewise)."""
    m = P("lpips")
    shape = (3, 3, 97, 131)
    rows = []
    for kind, close in (("close", True), ("far", False)):
        a, b = _pair(shape, 7 + int(close), normalize, close)
        mod = m.LPIPS(reduction=reduction, normalize=normalize, dtype=dtype)
        scale = mod._grad_scale(shape[0], mod.tap_sizes(97, 131))
        ref = _ref_grads(a, b, reduction, normalize)
        floor = _ref_grads(a, b, reduction, normalize, storage=dtype, scale=scale)
        got = {}
        for chunk in (None, 1):
            mod.max_pairs_per_launch = chunk
            x, y = a.to(dev).requires_grad_(), b.to(dev).requires_grad_()
            mod(x, y).backward()
            got[chunk] = (x.grad.cpu(), y.grad.cpu())
            for name, gh, gr, gf in zip(("img1", "img2"), got[chunk], ref, floor):
                c, cf = parity_util.cos(gh, gr), parity_util.cos(gf, gr)
                ratio, ratio_f = float(gh.double().norm() / gr.norm()), float(gf.norm() / gr.norm())
                row = (kind, name, "chunked" if chunk else "whole", f"1-cos={1 - c:.3e}", f"floor={1 - cf:.3e}",
                       f"ratio={ratio:.5f}", f"floor_ratio={ratio_f:.5f}")
                rows.append(row)
                print(dtype, normalize, reduction, *row)
                assert (1 - c) <= 1.5 * (1 - cf) + 0.01 and abs(ratio - 1) <= 0.03, row
        rel = 2.0 ** -8 if dtype == torch.float16 else 2.0 ** -5
        for whole, chunked in zip(got[None], got[1]):
            assert float((whole - chunked).abs().max()) <= rel * float(whole.abs().max()), (kind, rows)


def test_first_order_consistency_against_the_reference(dev):
    """A step t along -x.grad (the HIP gradient) changes the float64 reference value by -t |g|^2 up to second order.  t is
    chosen on the CPU from the float64 reference alone: the largest power of two for which a step along the reference's own
    gradient has a remainder under 10 % of t |g_ref|^2.  The HIP gradient may differ from the reference's by what the parity
    rule allows (3 % in norm, 1 - cos of about 0.01: together under 5 % of t |g|^2), so the bar is 15 %."""
    m = P("lpips")
    net, lins = _weights()
    a, b = _pair((2, 3, 80, 100), 17, close=False)
    val = lambda x: float(lpips_ref.lpips_per_image(x, b, net, lins).mean())
    g_ref, _ = _ref_grads(a, b, "mean", False)
    v0 = val(a.double())
    t = 2.0 ** 20
    while True:
        d = val(a.double() - t * g_ref) - v0
        if abs(d + t * float(g_ref.pow(2).sum())) <= 0.1 * t * float(g_ref.pow(2).sum()):
            break
        t /= 2
        assert t > 2.0 ** -40
    x = a.to(dev).requires_grad_()
    m.LPIPS()(x, b.to(dev)).backward()
    g = x.grad.cpu().double()
    d = val(a.double() - t * g) - v0
    g2 = float(g.pow(2).sum())
    print(f"t={t:g} delta={d:.6e} -t|g|^2={-t * g2:.6e} value={v0:.6e}")
    assert d < 0 and abs(d + t * g2) <= 0.15 * t * g2, (t, d, -t * g2)


def test_identical_inputs_give_zero_gradient_and_swap_swaps(dev):
    m = P("lpips")
    a, b = _pair((2, 3, 64, 72), 6, close=False)
    for dtype in (torch.float16, torch.bfloat16):
        mod = m.LPIPS(dtype=dtype)
        x, y = a.to(dev).requires_grad_(), a.to(dev).clone().requires_grad_()
        mod(x, y).backward()
        assert bool((x.grad == 0).all()) and bool((y.grad == 0).all())        # zero, not NaN
        x, y = a.to(dev).requires_grad_(), b.to(dev).requires_grad_()
        mod(x, y).backward()
        y2, x2 = b.to(dev).requires_grad_(), a.to(dev).requires_grad_()
        mod(y2, x2).backward()
        # the distance kernel's two halves are mirror images of one another bit for bit; behind it the images sit in the other
        # half of the convolutions' batch, which may change a tile and with it an accumulation order (see the chunked bar)
        rel = 2.0 ** -8 if dtype == torch.float16 else 2.0 ** -5
        for p, q in ((x.grad, x2.grad), (y.grad, y2.grad)):
            assert float((p - q).abs().max()) <= rel * float(p.abs().max())
        # one-sided and two-sided calls agree on the side they share
        x1 = a.to(dev).requires_grad_()
        mod(x1, b.to(dev)).backward()
        assert float((x1.grad - x.grad).abs().max()) <= rel * float(x.grad.abs().max())
        y1 = b.to(dev).requires_grad_()
        mod(a.to(dev), y1).backward()
        assert float((y1.grad - y.grad).abs().max()) <= rel * float(y.grad.abs().max())


def test_per_image_upstream_and_loss_weights(dev):
    """per_image with a different upstream weight per image, and a weighted scalar: the gradient is linear in what arrives."""
    m, F = P("lpips"), P("functional")
    a, b = _pair((3, 3, 64, 64), 23, close=False)
    mod = m.LPIPS(grad_scale=2.0 ** 16)
    x = a.to(dev).requires_grad_()
    wts = torch.tensor([1.0, 0.0, 0.5], device=dev)
    mod.per_image(x, b.to(dev)).backward(wts)
    ref, _ = _ref_grads(a, b, "sum", False)
    for i, wt in enumerate((1.0, 0.0, 0.5)):
        if wt == 0.0:
            assert bool((x.grad[i] == 0).all())
        else:
            assert parity_util.cos(x.grad[i].cpu(), ref[i]) > 0.99
            assert abs(float(x.grad[i].double().norm().cpu() / (wt * ref[i].norm())) - 1) < 0.03
    x2 = a.to(dev).requires_grad_()
    F.scale_loss(m.LPIPS(reduction="sum", grad_scale=2.0 ** 16)(x2, b.to(dev)), 0.25).backward()
    full, _ = _ref_grads(a, b, "sum", False)
    assert parity_util.cos(x2.grad.cpu(), full) > 0.99
    assert abs(float(x2.grad.double().norm().cpu() / (0.25 * full.norm())) - 1) < 0.03


def test_launch_log_of_forward_and_backward(dev, monkeypatch):
    """One forward + backward with only img1 requiring a gradient: one distance backward, two pool backwards, one stem
    backward, five input-gradient convolutions, no weight gradient -- and every backward descriptor has batch N, not 2N."""
    L, m = P("_lib"), P("lpips")
    mod = m.LPIPS()
    n = 2
    a, b = _pair((n, 3, 64, 64), 3)
    x = a.to(dev).requires_grad_()
    mod(x, b.to(dev)).backward()                       # packs both weight images outside the log
    lib = L.lib()
    batches = []
    for name in ("dsr_conv_dgrad", "dsr_conv_dgrad_masked"):
        inner = getattr(lib, name)

        def spy(*args, _inner=inner):
            batches.append(args[0]._obj.N)
            return _inner(*args)

        monkeypatch.setattr(lib, name, spy)
    pool_n = []
    inner_pool = lib.dsr_maxpool3s2_bwd
    monkeypatch.setattr(lib, "dsr_maxpool3s2_bwd", lambda *args: (pool_n.append(args[5]), inner_pool(*args))[1])
    x.grad = None
    L.LAUNCH_LOG = []
    try:
        mod(x, b.to(dev)).backward()
        torch.cuda.synchronize()
        names = [e[0] for e in L.LAUNCH_LOG]
    finally:
        L.LAUNCH_LOG = None
    assert names.count("dsr_lpips_distance_bwd") == 1
    assert names.count("dsr_maxpool3s2_bwd") == 2
    assert names.count("dsr_lpips_stem_prep_bwd") == 1
    assert names.count("dsr_conv_dgrad") + names.count("dsr_conv_dgrad_masked") == 5
    assert not [k for k in names if "wgrad" in k]
    assert batches == [n] * 5 and pool_n == [n] * 2, (batches, pool_n)
    # the forward half of the same call is what test_gpu_lpips.py::test_launch_log_of_one_call counts
    assert names.count("dsr_lpips_stem_prep") == 1 and names.count("dsr_conv_fwd") == 5 and names.count("dsr_maxpool3s2_fwd") == 2


def test_validate_range_switch(dev):
    m = P("lpips")
    a = torch.rand(1, 3, 64, 64, device=dev)
    with pytest.raises(ValueError, match="got values in"):
        m.LPIPS()(a * 3 - 1, a)
    with pytest.raises(ValueError, match="got values in"):
        m.LPIPS()((a * 3 - 1).requires_grad_(), a)
    out = m.LPIPS(validate_range=False)((a * 3 - 1).requires_grad_(), a)        # unchecked, by request
    assert bool(torch.isfinite(out))


# ============================================================================= the step recipe
def _make_step(dev, lpips_kw, step_kw, lr_rate=1e-3):
    from oracle import filler, gan
    Gm, optim, steps, m = P("models.GAN.generator"), P("optim"), P("steps"), P("lpips")
    sd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    lr = filler.tensor("in:lp_lr", (2, 3, 16, 16), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:lp_hr", (2, 3, 64, 64)).clamp(-1, 1).to(dev)
    g = Gm.Generator(4, 2)
    g.load_state_dict(sd)
    g.to(dev).train()
    opt = optim.FusedAdam(g.parameters(), lr=lr_rate)
    lp = m.LPIPS(**lpips_kw)
    return g, lp, hr, (lambda: steps.gen_lpips_step(g, opt, lp, lr, hr, **step_kw))


def test_gen_lpips_step_graphed_equals_eager(dev):
    """steps.gen_lpips_step: two steps replayed from a HIP graph (validate_range=False: a host read would fail the capture)
    leave bit for bit what the same number of eager steps leaves, and return the same loss terms."""
    steps = P("steps")
    g_e, _, _, step_e = _make_step(dev, dict(validate_range=False), {})
    for _ in range(4):
        out_e = step_e()
    g_g, _, _, step_g = _make_step(dev, dict(validate_range=False), {})
    graphed = steps.GraphedStep(step_g, warmup=2)         # 2 eager warm-up steps; capture itself executes nothing
    for _ in range(2):
        out_g = graphed()
    torch.cuda.synchronize()
    assert len(out_e) == len(out_g) == 3
    for p, q in zip(out_e, out_g):
        assert torch.equal(p, q)
    for (k, p), (_, q) in zip(g_e.state_dict().items(), g_g.state_dict().items()):
        assert torch.equal(p, q), k


def test_gen_lpips_step_returns_the_metric_and_lowers_it(dev):
    """The returned LPIPS term is LPIPS.forward of the same images; minimising LPIPS alone (l1_weight = 0) for 20 Adam steps
    on one fixed batch lowers it (last < first; monotonic decrease is not required), and the default weighting does too."""
    _, lp, hr, step = _make_step(dev, {}, {})
    l1, val, fake = step()
    assert l1.shape == () and val.shape == () and fake.shape == hr.shape
    assert torch.equal(val, lp(fake, hr))
    assert abs(float(l1) - float((fake - hr).abs().mean())) <= 1e-5 * float(l1)
    for kw in (dict(l1_weight=0.0, lpips_weight=1.0), {}):
        _, _, _, step = _make_step(dev, {}, kw, lr_rate=5e-4)
        vals = [float(step()[1]) for _ in range(20)]
        print("LPIPS over 20 steps", kw, [round(v, 5) for v in vals])
        assert vals[-1] < vals[0], vals
