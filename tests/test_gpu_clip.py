"""GPU: device-side gradient-norm clipping and the tensor learning rate of optim.FusedAdam (dsr_clip_sumsq,
dsr_linear_factor_gram, dsr_clip_finalize and the Adam entry points with dsr_adam_args.hyper set).

The reference project has neither clipping nor a schedule; the yardstick is torch itself: torch.nn.utils.clip_grad_norm_
followed by torch.optim.Adam, modelled in float64 by tests/clip_ref.py (which tests/test_host_clip.py checks against torch).
Inf is an ordinary float value in a buffer here; nothing in this file can fault the device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import clip_ref
from adam_args import adam_args
from oracle import dip, downsampler, filler, gan

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
E_UNSUPPORTED = -4


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def all_same(xs, ys):
    return len(xs) == len(ys) and all(same(a, b) for a, b in zip(xs, ys))


def table(tensors):
    k = len(tensors)
    return (k, (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in tensors]),
            (C.c_size_t * k)(*[0 if t is None else t.numel() for t in tensors]))


# ----------------------------------------------------------------------------- 1: sum of squares
def device_norm(tensors, dev, grad_scale=1.0, scale=None, max_norm=1.0):
    """dsr_clip_sumsq + dsr_clip_finalize: (norm, coef, raw partials)."""
    L = P("_lib")
    lib = L.lib()
    k, ptrs, ns = table(tensors)
    n = lib.dsr_clip_sumsq_partials(k, ptrs, ns)
    assert n > 0
    parts = torch.full((n + 8,), float("nan"), device=dev)            # the 8 behind the last partial must stay untouched
    L.check(lib.dsr_clip_sumsq(k, ptrs, ns, ptr(parts), n, stream()))
    norm, coef, hyper = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.zeros(2, device=dev)
    L.check(lib.dsr_clip_finalize(ptr(parts), n, None, 0, grad_scale, ptr(scale), max_norm, None, 0.25, ptr(norm), ptr(coef),
                                  ptr(hyper), stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(parts[n:]).all()) and bool(torch.isfinite(parts[:n]).all())
    assert hyper[0].item() == 0.25 and same(hyper[1:], coef)
    return norm.item(), coef.item(), parts[:n].clone()


def test_sum_of_squares_against_float64(dev):
    """Bar 2e-6 on the norm, from the accumulation scheme of clip_sumsq_kernel: all terms are non-negative, so nothing cancels
    and relative errors do not grow; a thread squares (one rounding each) and adds in fp32 at most 32 body elements and 2 head
    or tail elements in sequence, i.e. fewer than 64 roundings of 2^-24 on its sum; from the thread sums upwards everything is
    fp64 except ONE rounding of the block partial to fp32.  That is < 64 * 2^-24 = 3.8e-6 relative on the sum of squares and
    half of it, 1.9e-6, on its root; the fp32 rounding of the result itself (6e-8) fits in the slack to 2e-6."""
    g = torch.Generator(device="cpu").manual_seed(23)
    sizes = (1, 3, 7, 4096, (1 << 20) + 5)
    tensors = []
    for off in (0, 1, 2, 3):                                  # views 0 / 4 / 8 / 12 bytes off a 16-byte boundary
        for n in sizes:
            t = (torch.randn(n + off, generator=g) * (0.1 + off)).to(dev)[off:]
            assert t.numel() == n and t.data_ptr() % 16 == 4 * off
            tensors.append(t)
    tensors = tensors[:7] + [None] + tensors[7:] + [torch.randn(5, generator=g).to(dev) for _ in range(64)]
    assert len(tensors) > 64 and any(t is None for t in tensors)
    want = clip_ref.total_norm([None if t is None else t.cpu().numpy() for t in tensors])
    norm, coef, parts = device_norm(tensors, dev)
    err = abs(norm - want) / want
    print(f"\nsum of squares over {len(tensors)} ragged tensors: norm {norm:.9g}, float64 {want:.9g}, relative error {err:.3e}")
    assert err <= 2e-6
    assert abs(coef - 1.0 / (want + 1e-6)) <= 4e-6 * coef and coef < 1.0
    norm2, coef2, parts2 = device_norm(tensors, dev)
    assert norm2 == norm and coef2 == coef and same(parts, parts2)          # no atomics: the same bits on every run
    # the scale regimes: static grad_scale (norm x |grad_scale|), the loss scaler's device word (norm / scale[0]), no clipping
    n3, c3, _ = device_norm(tensors, dev, grad_scale=-1.0 / 1024)
    assert abs(n3 - want / 1024) <= 2e-6 * want / 1024 and abs(c3 - 1.0 / (want / 1024 + 1e-6)) <= 4e-6 * c3
    n4, _, _ = device_norm(tensors, dev, grad_scale=1.0, scale=torch.full((1,), 4096.0, device=dev))
    assert abs(n4 - want / 4096) <= 2e-6 * want / 4096
    assert device_norm(tensors, dev, max_norm=0.0)[1] == 1.0 and device_norm(tensors, dev, max_norm=1e30)[1] == 1.0
    # Inf and NaN are values like any other: Inf norm -> coefficient 0, NaN -> NaN, as torch forms them
    keep = tensors[4][77].clone()
    tensors[4][77] = float("inf")
    L = P("_lib")
    k, ptrs, ns = table(tensors)
    n = L.lib().dsr_clip_sumsq_partials(k, ptrs, ns)
    parts = torch.zeros(n, device=dev)
    L.check(L.lib().dsr_clip_sumsq(k, ptrs, ns, ptr(parts), n, stream()))
    nrm, cf, hy = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.zeros(2, device=dev)
    L.check(L.lib().dsr_clip_finalize(ptr(parts), n, None, 0, 1.0, None, 1.0, None, 0.5, ptr(nrm), ptr(cf), ptr(hy), stream()))
    assert nrm.item() == float("inf") and cf.item() == 0.0
    tensors[4][77] = float("nan")
    L.check(L.lib().dsr_clip_sumsq(k, ptrs, ns, ptr(parts), n, stream()))
    L.check(L.lib().dsr_clip_finalize(ptr(parts), n, None, 0, 1.0, None, 1.0, None, 0.5, ptr(nrm), ptr(cf), ptr(hy), stream()))
    assert np.isnan(nrm.item()) and np.isnan(cf.item())
    tensors[4][77] = keep


# ----------------------------------------------------------------------------- 2: Gram norm of the factored gradient
def _factors(dev, o, k, bp, r, batch, dtype, seed):
    """[R][O][Bp] and [R][K][Bp] factor tables with the columns beyond the batch zero, as DenseHead.backward leaves them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dyt = torch.zeros(r, o, bp)
    xt = torch.zeros(r, k, bp)
    dyt[:, :, :batch] = torch.randn(r, o, batch, generator=g) * 0.02
    xt[:, :, :batch] = torch.randn(r, k, batch, generator=g).abs() * 0.5 - 0.1      # a LeakyReLU-like, mostly positive activation
    return dyt.to(dtype).to(dev), xt.to(dtype).to(dev)


def _truth_norm(dyt, xt, scale):
    """float64 norm of scale * sum_r dyT_r xT_r^T from the exact 16-bit values (via the two Gram matrices, in float64)."""
    r, o, bp = dyt.shape
    a = dyt.double().cpu().permute(1, 0, 2).reshape(o, r * bp)
    b = xt.double().cpu().permute(1, 0, 2).reshape(xt.shape[1], r * bp)
    return abs(scale) * float(((a.t() @ a) * (b.t() @ b)).sum().sqrt())


def gram_norm(dyt, xt, scale, dev):
    L = P("_lib")
    lib = L.lib()
    r, o, bp = dyt.shape
    k = xt.shape[1]
    dt = 0 if dyt.dtype == torch.bfloat16 else 1
    nbytes = lib.dsr_linear_factor_gram_workspace(bp, o, k, r)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.dsr_linear_factor_gram(dt, ptr(dyt), ptr(xt), bp, o, k, r, scale, ptr(ws), nbytes, stream()))
    nd = lib.dsr_linear_factor_gram_dots(bp, r)
    norm, hyper = torch.zeros(1, device=dev), torch.zeros(2, device=dev)
    L.check(lib.dsr_clip_finalize(None, 0, ptr(ws), nd, 1.0, None, 1.0, None, 0.5, ptr(norm), None, ptr(hyper), stream()))
    torch.cuda.synchronize()
    return norm.item(), ws[:8 * nd].view(torch.float64).clone()


@pytest.mark.parametrize("bp,r,batch,dtype", [(32, 1, 20, torch.bfloat16), (64, 1, 40, torch.bfloat16), (32, 2, 17, torch.bfloat16),
                                              (64, 2, 64, torch.float16), (32, 3, 32, torch.bfloat16)])
def test_gram_norm_against_the_materialised_gradient(dev, bp, r, batch, dtype):
    """D at 192x192: O = 1024, K = 73,728.  Truth: float64 from the exact 16-bit factor values.  Yardstick: how far the norm of
    the fp32 gradient that dsr_linear_wgrad / dsr_linear_wgrad_gathered produce is from that truth; the Gram norm may be at
    most 4 x as far (room for a different summation order), with a floor of 1e-6 relative.
    Measured on the MI355X (relative deviation from the truth, Gram norm / norm of the materialised gradient):
    Bp 32 R 1: 1.9e-8 / 1.4e-11; Bp 64 R 1: 9.4e-10 / 1.0e-11; Bp 32 R 2: 1.4e-8 / 1.0e-11; Bp 64 R 2 (f16): 7.0e-9 / 3.3e-10;
    Bp 32 R 3: 5.8e-8 / 2.9e-8 -- the Gram norm meets the bar through the 1e-6 floor, not through the factor 4."""
    F = P("functional")
    o, k = 1024, 73728
    dyt, xt = _factors(dev, o, k, bp, r, batch, dtype, 100 + bp + r)
    scale = 1.0 / r
    want = _truth_norm(dyt, xt, scale)
    dt = 0 if dtype == torch.bfloat16 else 1
    fac = F.GradFactors(dt, dyt if r > 1 else dyt[0], xt if r > 1 else xt[0], bp, o, k, r, scale, ())
    dw = fac.materialize()
    yard = abs(float(dw.double().norm()) - want) / want
    got, dots = gram_norm(dyt, xt, scale, dev)
    err = abs(got - want) / want
    print(f"\nGram norm Bp={bp} R={r} batch={batch} {dtype}: {got:.9g} vs float64 {want:.9g}: relative {err:.3e}; "
          f"materialised fp32 gradient {yard:.3e}")
    assert err <= max(4 * yard, 1e-6)
    got2, dots2 = gram_norm(dyt, xt, scale, dev)
    assert got2 == got and bool((dots == dots2).all())                       # bit-reproducible


def test_gram_norm_beyond_512_rows_falls_back(dev):
    """R * Bp > 512: the C entry answers DSR_E_UNSUPPORTED, FusedAdam materialises the gradient and takes the tensor pass; the
    norm meets the same bar against the float64 truth."""
    O, F, L = P("optim"), P("functional"), P("_lib")
    o, k, bp, r = 64, 256, 64, 9
    dyt, xt = _factors(dev, o, k, bp, r, 33, torch.bfloat16, 7)
    one = torch.zeros(64, device=dev)
    assert L.lib().dsr_linear_factor_gram(0, ptr(dyt), ptr(xt), bp, o, k, r, 1.0, ptr(one), 1 << 20, stream()) == E_UNSUPPORTED
    want = _truth_norm(dyt, xt, 1.0 / r)
    for rows, (d_, x_) in ((r, (dyt, xt)), (8, (dyt[:8].contiguous(), xt[:8].contiguous()))):      # fallback, then 512 rows: Gram
        sc = 1.0 / rows
        w = torch.zeros(o, k, device=dev, requires_grad=True)
        w._dsr_grad_factors = [F.GradFactors(0, d_, x_, bp, o, k, rows, sc, ())]
        opt = O.FusedAdam([w], lr=1e-3, max_grad_norm=1e-3, fuse_dense_head=True)
        opt.step()
        torch.cuda.synchronize()
        truth = _truth_norm(d_, x_, sc)
        dw = F.GradFactors(0, d_, x_, bp, o, k, rows, sc, ()).materialize()
        yard = abs(float(dw.double().norm()) - truth) / truth
        err = abs(opt.grad_norm.item() - truth) / truth
        print(f"\nR*Bp = {rows * bp}: FusedAdam.grad_norm relative {err:.3e}, materialised {yard:.3e}")
        assert err <= max(4 * yard, 1e-6)
        assert w.grad is None and bool((w != 0).any())
    assert want > 0


# ----------------------------------------------------------------------------- 3: optimiser parity
def _ragged(dev):
    shapes = [(1 + (7 * i) % 33, 1 + (5 * i) % 19) for i in range(149)] + [(9000,)]       # test_adam_multi_tensor_matches_per_tensor
    w0 = [filler.tensor(f"am:w{i}", s) for i, s in enumerate(shapes)]
    targets = (0.5, 50.0, 0.5, 3.0, 0.2)                    # norms on both sides of max_grad_norm = 1
    grads = []
    for it, tn in enumerate(targets):
        gs = [filler.tensor(f"am:g{it}:{i}", s) for i, s in enumerate(shapes)]
        nrm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
        grads.append([(g * (tn / nrm)).float() for g in gs])
    return shapes, w0, grads, targets


def _rel(a, b):
    a = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in a])
    b = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in b])
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_clipped_adam_against_float64_reference(dev):
    """Bar: the larger of 1e-6 relative (the Adam parity bar of tests/test_gpu_kernels.py) and 4 x the deviation of torch's own
    fp32 CPU clip_grad_norm_ + Adam from the float64 model on the same inputs.  Clipped and unclipped trajectories must be at
    least 100 x that bar apart, or the comparison would show nothing."""
    O = P("optim")
    shapes, w0, grads, targets = _ragged(dev)
    lr, c = 3e-3, 1.0
    ref = clip_ref.ClippedAdam([w.numpy() for w in w0], lr=lr, max_grad_norm=c)
    free = clip_ref.ClippedAdam([w.numpy() for w in w0], lr=lr)
    tp = [w.clone().requires_grad_(True) for w in w0]
    topt = torch.optim.Adam(tp, lr=lr)
    runs = []
    for multi_max in (None, 0):                              # the multi-tensor launch, then per-tensor launches
        ps = [w.to(dev).requires_grad_(True) for w in w0]
        opt = O.FusedAdam(ps, lr=lr, max_grad_norm=c)
        if multi_max is not None:
            opt.MULTI_MAX = multi_max
        runs.append((ps, opt))
    for it, gs in enumerate(grads):
        ref.step([g.numpy() for g in gs])
        free.step([g.numpy() for g in gs])
        for p, g in zip(tp, gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(tp, c)
        topt.step()
        for ps, opt in runs:
            for p, g in zip(ps, gs):
                p.grad = g.to(dev)
            opt.step()
            gn, cc = opt.grad_norm.item(), opt.clip_coef.item()
            assert abs(gn - ref.grad_norm) <= 2e-6 * ref.grad_norm, (it, gn, ref.grad_norm)
            assert abs(cc - ref.clip_coef) <= 4e-6 * ref.clip_coef, (it, cc, ref.clip_coef)
            assert (cc == 1.0) == (targets[it] < c)
            assert all(same(p.grad, g.to(dev)) for p, g in zip(ps[:5], gs[:5]))          # the gradients are not rewritten
    torch.cuda.synchronize()
    floor = _rel([p.detach().numpy() for p in tp], ref.p)
    bar = max(1e-6, 4 * floor)
    apart = _rel(free.p, ref.p)
    print(f"\nclipped Adam, {len(grads)} steps: torch fp32 vs float64 {floor:.3e} -> bar {bar:.3e}; clipped vs unclipped {apart:.3e}")
    assert apart >= 100 * bar
    for ps, opt in runs:
        err = _rel([p.detach().cpu().numpy() for p in ps], ref.p)
        print(f"  FusedAdam(MULTI_MAX={opt.MULTI_MAX}) vs float64: {err:.3e}")
        assert err <= bar


# ----------------------------------------------------------------------------- 4: identity cases
def _state(ps, opt):
    return [bits(p) for p in ps] + [bits(t) for t in opt.m + opt.v] + [bits(opt.step_t)]


def _run_plain(dev, w0, grads, multi_max=None, **kw):
    O, L = P("optim"), P("_lib")
    ps = [w.to(dev).requires_grad_(True) for w in w0]
    opt = O.FusedAdam(ps, **kw)
    if multi_max is not None:
        opt.MULTI_MAX = multi_max
    names = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dev)
        L.LAUNCH_LOG = []
        try:
            opt.step()
            names.append([n for n, _, _ in L.LAUNCH_LOG])
        finally:
            L.LAUNCH_LOG = None
    torch.cuda.synchronize()
    return _state(ps, opt), names, opt


def test_identity_cases_are_bit_equal(dev):
    shapes, w0, grads, _ = _ragged(dev)
    w0, grads = w0[100:], [g[100:] for g in grads]           # 50 tensors, the 9000-element one among them
    for mm in (None, 64):                                    # 64: most tensors take the per-tensor launch
        base, names, _ = _run_plain(dev, w0, grads, mm, lr=3e-3)
        n_big = sum(1 for w in w0 if w.numel() > (mm if mm is not None else 1 << 20))
        # both features off: the launches of the parent commit -- the counter, one dsr_pw_adam per big tensor, one multi launch
        want = ["dsr_pw_incr"] + ["dsr_pw_adam"] * n_big + ["dsr_pw_adam_multi"]
        assert all(n == want for n in names), names[0]
        huge, hn, _ = _run_plain(dev, w0, grads, mm, lr=3e-3, max_grad_norm=1e30)
        assert all_same(huge, base)                          # a bound never reached: the coefficient is exactly 1
        assert hn[0] == ["dsr_pw_incr", "dsr_clip_sumsq", "dsr_clip_finalize"] + ["dsr_pw_adam"] * n_big + ["dsr_pw_adam_multi"]
        tl, tn, opt = _run_plain(dev, w0, grads, mm, lr=torch.tensor(3e-3, device=dev))
        assert all_same(tl, base)                            # a tensor lr holding the fp32 value of the float
        assert tn[0] == ["dsr_pw_incr", "dsr_clip_finalize"] + ["dsr_pw_adam"] * n_big + ["dsr_pw_adam_multi"]
        both, _, _ = _run_plain(dev, w0, grads, mm, lr=torch.tensor(3e-3), max_grad_norm=1e30)
        assert all_same(both, base)
        clipped, _, _ = _run_plain(dev, w0, grads, mm, lr=3e-3, max_grad_norm=1.0)
        assert not all_same(clipped, base)
    # the static grad_scale rides in the one fp32 product grad_scale * coef
    sbase, _, _ = _run_plain(dev, w0, [[g * 1024 for g in gs] for gs in grads], lr=3e-3, grad_scale=1.0 / 1024)
    shuge, _, so = _run_plain(dev, w0, [[g * 1024 for g in gs] for gs in grads], lr=3e-3, grad_scale=1.0 / 1024, max_grad_norm=1e30)
    assert all_same(shuge, sbase)
    want_norm = clip_ref.total_norm([g.numpy() for g in grads[-1]])
    assert abs(so.grad_norm.item() - want_norm) <= 2e-6 * want_norm          # the norm of the TRUE gradient


# ----------------------------------------------------------------------------- 5: dense head
def test_dense_head_clipping_without_the_gradient(dev):
    """Discriminator((64, 64)), loss_D backward: FusedAdam(fuse_dense_head=True, max_grad_norm=c) never holds dense1's gradient
    and must agree with fuse_dense_head=False (norm: the bar of the Gram test against the tensor pass; parameters: the bar of
    the parity test) and with torch.nn.utils.clip_grad_norm_ on the materialised gradients."""
    O, Dm, F = P("optim"), P("models.GAN.discriminator"), P("functional")
    dsd = filler.fill_state_dict(gan.template(gan.discriminator_shapes((64, 64))))
    real = filler.tensor("in:clip_real", (4, 3, 64, 64)).to(dev)
    fake = filler.tensor("in:clip_fake", (4, 3, 64, 64), 0.3).to(dev)
    c = 1e-3

    def run(fuse, steps=3):
        F.clear_pack_cache()
        d = Dm.Discriminator((64, 64))
        d.load_state_dict(dsd)
        d.to(dev).train()
        opt = O.FusedAdam(d.parameters(), lr=1e-4, fuse_dense_head=fuse, max_grad_norm=c)
        rows = []
        for _ in range(steps):
            real_d, fake_d = d.forward_pair(real, fake)
            loss = F.add_losses(F.bce_const(real_d, 1.0), F.bce_const(fake_d, 0.0))
            opt.zero_grad()
            loss.backward()
            gs = [p.grad.detach().clone() for p in d.parameters() if p.grad is not None]
            bar = 2e-6                                        # the tensor pass (test_sum_of_squares_against_float64)
            if fuse:
                assert d.dense1.weight.grad is None and len(d.dense1.weight._dsr_grad_factors) == 1
                f = d.dense1.weight._dsr_grad_factors[0]
                dense = _truth_norm(f.dyt[None], f.xt[None], f.scale)
                dw = f.materialize()                          # what torch's clip_grad_norm_ has to be given
                yard = abs(float(dw.double().norm()) - dense) / dense
                bar += max(4 * yard, 1e-6)                    # plus the Gram pass (test_gram_norm_against_the_materialised_gradient)
                truth = float(np.sqrt(dense ** 2 + sum(float((g.double() ** 2).sum()) for g in gs)))
                gs.append(dw)
            else:
                assert d.dense1.weight.grad is not None
                truth = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in gs)))
            holders = []
            for g in gs:
                q = torch.nn.Parameter(torch.zeros_like(g))
                q.grad = g
                holders.append(q)
            tnorm = float(torch.nn.utils.clip_grad_norm_(holders, 1e30))      # torch's own norm of the materialised gradients
            opt.step()
            rows.append((opt.grad_norm.item(), opt.clip_coef.item(), tnorm, truth, bar))
        torch.cuda.synchronize()
        return d, rows

    d_f, rows_f = run(True)
    d_t, rows_t = run(False)
    for it, (rf, rt) in enumerate(zip(rows_f, rows_t)):
        for name, (gn, cf, tn, truth, bar) in (("fused", rf), ("tensor pass", rt)):
            print(f"\ndense head step {it}, {name}: grad_norm {gn:.9g}, float64 {truth:.9g}, torch on the materialised gradients "
                  f"{tn:.9g}; coef {cf:.4g}; bar {bar:.2e}")
            assert cf < 1.0                                   # clipping is active on every step
            assert abs(gn - truth) <= bar * truth
            assert abs(gn - tn) <= (bar + 2e-6) * tn          # torch's fp32 norm carries a rounding error of its own
            assert abs(cf - c / (tn + 1e-6)) <= (bar + 4e-6) * cf
    # the first step sees identical weights and batch on both routes
    assert abs(rows_f[0][0] - rows_t[0][0]) <= (rows_f[0][4] + rows_t[0][4]) * rows_t[0][0]
    pf = [p.detach().cpu().numpy() for p in d_f.parameters()]
    pt = [p.detach().cpu().numpy() for p in d_t.parameters()]
    err = _rel(pf, pt)
    print(f"dense head: parameters after 3 clipped steps, fused vs separate: {err:.3e}")
    assert err <= 1e-6                                        # the Adam parity bar (no wider: torch's fp32 deviation is not measured here)


# ----------------------------------------------------------------------------- 6: scaler
def _dip(dev, loss_scale, max_grad_norm, size=64):
    M, D, steps = P("models.DIP"), P("utils.downsampler"), P("steps")
    P("functional").clear_pack_cache()
    sd = filler.fill_state_dict(gan.template(dip.skip_shapes(dip.SkipConfig(input_depth=32))))
    net = M.get_net(32, "skip", "reflection", upsample_mode="bilinear")
    net.load_state_dict(sd)
    net.to(dev).train()
    assert net.compute_dtype == torch.float16
    down = D.Downsampler(3, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
    hr = filler.tensor("in:clip_dip_hr", (1, 3, size, size), 0.5, 0.5)
    lr_img = downsampler.downsampler_forward(hr, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
    zin = filler.tensor("in:clip_dip_z", (1, 32, size, size), 0.05, 0.05).to(dev)
    return steps.DipRunner(net, down, zin, lr_img, 0.01, 0.05, loss_scale=loss_scale, max_grad_norm=max_grad_norm)


def _dip_noise(it, dev, size=64):
    return filler.tensor(f"in:clip_dip_noise{it}", (1, 32, size, size), 1.7).to(dev)


def _dip_state(run):
    return [bits(p) for p in run.net.parameters()] + [bits(t) for t in run.opt.m + run.opt.v] + [bits(run.opt.step_t)]


def test_dip_clipping_under_the_dynamic_scaler(dev):
    O = P("optim")
    probe = _dip(dev, 1024.0, 1e30)
    probe.step(_dip_noise(0, dev))
    true_norm = probe.opt.grad_norm.item()                    # of the un-scaled gradient (grad_scale = 1 / 1024 taken out)
    assert 0.0 < true_norm < float("inf")
    other = _dip(dev, 256.0, 1e30)                            # another scale: the same true gradient up to fp16 rounding; a scale
    other.step(_dip_noise(0, dev))                            # left in the norm would show as the factor 4 between the two
    assert abs(other.opt.grad_norm.item() - true_norm) <= 0.25 * true_norm
    c = true_norm / 4                                         # active on the first step
    stat = _dip(dev, 1024.0, c)
    dyn_sc = O.DynamicLossScaler(init_scale=1024.0, growth_interval=10 ** 9)
    dyn = _dip(dev, dyn_sc, c)
    assert dyn.scaler is dyn_sc and dyn.opt.max_grad_norm == c
    for it in range(4):
        ls, outs = stat.step(_dip_noise(it, dev))
        ld, outd = dyn.step(_dip_noise(it, dev))
        assert same(ls, ld) and same(outs, outd), it
        assert same(stat.opt.grad_norm, dyn.opt.grad_norm) and same(stat.opt.clip_coef, dyn.opt.clip_coef), it
        if it == 0:
            assert same(stat.opt.grad_norm, probe.opt.grad_norm) and stat.opt.clip_coef.item() < 0.3
    assert all_same(_dip_state(stat), _dip_state(dyn))
    assert dyn_sc.counts() == (4, 0)
    unclipped = _dip(dev, 1024.0, None)
    for it in range(4):
        unclipped.step(_dip_noise(it, dev))
    assert not all_same(_dip_state(unclipped), _dip_state(stat))
    # an injected Inf: the step is skipped, nothing of the optimiser moves
    w = [torch.ones(300, device=dev, requires_grad=True), torch.ones(5000, device=dev, requires_grad=True)]
    opt = O.FusedAdam(w, lr=torch.tensor(1e-2), max_grad_norm=1.0)
    opt.MULTI_MAX = 1000                                      # one tensor per launch kind
    sc = O.DynamicLossScaler(init_scale=4.0, growth_interval=10 ** 9)
    for it in range(3):
        for p in w:
            p.grad = torch.full_like(p, (4.0 if it < 2 else 2.0) * 0.01)      # the scaled gradient of a true 0.01
        if it == 1:
            w[1].grad[4321] = float("inf")
        before = _state(w, opt)
        sc.step(opt)
        sc.update()
        assert all_same(before, _state(w, opt)) == (it == 1), it
    assert sc.counts() == (2, 1) and opt.step_t.item() == 2 and sc.get_scale() == 2.0
    want = 0.01 * np.sqrt(5300.0)
    assert abs(opt.grad_norm.item() - want) <= 2e-6 * want    # the un-scaled gradient's norm (scale 2 by now)


# ----------------------------------------------------------------------------- 7: graph replay
def test_graphed_step_reads_the_lr_tensor(dev):
    O, S, F = P("optim"), P("steps"), P("functional")
    gen = P("models.GAN.generator")
    lr_in = filler.tensor("in:traj_lr", (4, 3, 24, 24), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:traj_hr", (4, 3, 96, 96)).to(dev)
    lrs = (1e-3, 1e-4, 5e-4, 1e-5, 2e-3)                      # one warm-up step, then four replays

    def make():
        F.clear_pack_cache()
        g = gen.Generator(4, 2)
        g.load_state_dict(filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2))))
        g.to(dev).train()
        opt = O.FusedAdam(g.parameters(), lr=torch.tensor(lrs[0], device=dev), max_grad_norm=1e-3)
        return g, opt

    def state(g, opt):
        return [bits(p) for p in g.parameters()] + [bits(t) for t in opt.m + opt.v] + [bits(opt.step_t)]

    g_e, o_e = make()
    coefs = []
    for x in lrs:
        o_e.lr.fill_(x)
        S.gen_l1_step(g_e, o_e, lr_in, hr)
        coefs.append(o_e.clip_coef.item())
    assert min(coefs) < 1.0                                   # the clipping is at work in these steps
    results = {}
    for name, seq in (("scheduled", lrs), ("constant", (lrs[0],) * len(lrs))):
        g, opt = make()
        graphed = S.GraphedStep(lambda: S.gen_l1_step(g, opt, lr_in, hr), warmup=1)
        for x in seq[1:]:
            opt.lr.fill_(x)
            graphed()
        torch.cuda.synchronize()
        results[name] = state(g, opt)
    assert all_same(results["scheduled"], state(g_e, o_e))
    assert not all_same(results["constant"], results["scheduled"])


# ----------------------------------------------------------------------------- 8: bad arguments on the device side of the ABI
def test_bad_arguments_return_codes(dev):
    L = P("_lib")
    lib = L.lib()
    t = torch.zeros(64, device=dev)
    h16 = torch.zeros(64 * 64, dtype=torch.bfloat16, device=dev)
    N, st = None, stream()
    k, ptrs, ns = table([t, t])
    off = C.c_void_p(t.data_ptr() + 2)
    # the device-hyper mode of dsr_adam_args; a null hyper selects the plain mode, so the refused block has a misaligned one
    hy = lambda **kw: adam_args(**{**dict(step=t, hyper=t), **kw})
    calls = [
        lambda: lib.dsr_clip_sumsq(0, ptrs, ns, ptr(t), 64, st),
        lambda: lib.dsr_clip_sumsq(k, N, ns, ptr(t), 64, st),
        lambda: lib.dsr_clip_sumsq(k, ptrs, ns, N, 64, st),
        lambda: lib.dsr_clip_sumsq(k, ptrs, ns, ptr(t), 1, st),
        lambda: lib.dsr_clip_sumsq(k, ptrs, ns, off, 64, st),
        lambda: lib.dsr_clip_finalize(ptr(t), 2, N, 0, 1.0, N, 1.0, N, 1e-3, N, N, N, st),
        lambda: lib.dsr_clip_finalize(N, 2, N, 0, 1.0, N, 1.0, N, 1e-3, N, N, ptr(t), st),
        lambda: lib.dsr_clip_finalize(off, 2, N, 0, 1.0, N, 1.0, N, 1e-3, N, N, ptr(t), st),
        lambda: lib.dsr_pw_adam(ptr(t), ptr(t), ptr(t), ptr(t), 0, N, hy(), st),
        lambda: lib.dsr_pw_adam(ptr(t), ptr(t), ptr(t), ptr(t), 64, N, hy(hyper=off), st),
        lambda: lib.dsr_pw_adam(ptr(t), off, ptr(t), ptr(t), 16, N, hy(), st),
        lambda: lib.dsr_pw_adam_multi(0, ptrs, ptrs, ptrs, ptrs, ns, hy(), st),
        lambda: lib.dsr_pw_adam_multi(k, ptrs, N, ptrs, ptrs, ns, hy(), st),
        lambda: lib.dsr_pw_adam_multi(k, ptrs, ptrs, ptrs, ptrs, ns, hy(hyper=off), st),
        lambda: lib.dsr_linear_factor_gram(0, N, ptr(h16), 32, 8, 64, 1, 1.0, ptr(t), 256, st),
        lambda: lib.dsr_linear_factor_gram(0, ptr(h16), ptr(h16), 48, 8, 64, 1, 1.0, ptr(t), 256, st),
        lambda: lib.dsr_linear_factor_gram(0, ptr(h16), ptr(h16), 32, 8, 64, 1, 1.0, ptr(t), 256, st),      # short workspace
        lambda: lib.dsr_linear_factor_gram(0, ptr(h16), ptr(h16), 64, 8, 64, 9, 1.0, ptr(t), 256, st),
        lambda: lib.dsr_linear_factor_gram(0, off, ptr(h16), 32, 8, 64, 1, 1.0, ptr(t), 256, st),
        lambda: lib.dsr_linear_wgrad_adam(0, ptr(h16), ptr(h16), 16, 8, 64, 1, 1.0, ptr(t), ptr(t), ptr(t), N, hy(), st),
        lambda: lib.dsr_linear_wgrad_adam(0, ptr(h16), ptr(h16), 32, 8, 64, 1, 1.0, ptr(t), ptr(t), ptr(t), N, hy(hyper=off), st),
        lambda: lib.dsr_linear_wgrad_adam(0, ptr(h16), ptr(h16), 32, 8, 40, 1, 1.0, ptr(t), ptr(t), ptr(t), N, hy(), st),
        lambda: lib.dsr_linear_wgrad_adam(0, ptr(h16), ptr(h16), 32, 8, 64, 1, 1.0, off, ptr(t), ptr(t), N, hy(), st),
    ]
    for i, call in enumerate(calls):
        assert call() < 0, i
        assert lib.dsr_last_error(), i
    torch.cuda.synchronize()
    assert bool((t == 0).all())
