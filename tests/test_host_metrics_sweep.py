"""CPU: the metric sweep's references, exact regimes, case tables and floors (metrics_ref.py).  Nothing here launches a kernel.

The references are pinned against the restatements the suite already has (ssim_ref.py, msssim_ref.py, the float64 PSNR formula)
to 1e-12; every exact-regime case is shown to be exact in float32 in any order; the case tables are shown to reach every branch
the launchers and kernels of csrc/metrics.hip can take, with the tile sizes, the chunk and the finalisers' strides read from that
file as text; and the floor of every measured bar of test_gpu_metrics_sweep.py is computed and printed here too, so a change of
the inputs shows without a GPU."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as TF

import metrics_ref as R
import msssim_ref
import ssim_ref

PKG = "deep-super-resolution_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32


def _flat_src():
    return re.sub(r"\s+", "", open(os.path.join(ROOT, PKG, "csrc", "metrics.hip")).read())


# ----------------------------------------------------------------------------- the references are the restatements they build on
def test_tile_sums_fold_back_to_the_per_image_means():
    for shape in R.FWD_SHAPES:
        a, b = R.fwd_case(shape)
        n, c, h, w = shape
        count = c * (h - 10) * (w - 10)
        th, tw = R.SF_TH, R.SF_TW
        ref = R.fwd_reference(shape, th, tw)
        sim, cs = R.fwd_maps(a, b)
        s, cnt = R.tile_sums(sim, th, tw)
        q, _ = R.tile_sums(cs, th, tw)
        nblk = R.blocks_per_image(shape, th, tw)
        assert s.numel() == n * nblk and int(cnt.view(n, nblk).sum(1)[0]) == count and int(cnt.min()) >= 1
        assert float((s.view(n, nblk).sum(1) / count - ssim_ref.ssim_per_image(a, b)).abs().max()) <= 1e-12
        if min(h, w) >= 22:                               # two scales fit: row 0 is the cs mean of scale 0
            raw = msssim_ref.raw_scales(a, b, 2)
            assert float((q.view(n, nblk).sum(1) / count - raw[0]).abs().max()) <= 1e-12
        assert float((q.view(n, nblk).sum(1) / count - cs.mean(dim=(1, 2, 3))).abs().max()) <= 1e-12
        assert float((s.view(n, nblk).sum(1) / count - msssim_ref.raw_scales(a, b, 1)[0]).abs().max()) <= 1e-12
        assert torch.equal(ref["sim"], s) and torch.equal(ref["cnt"], cnt)
    # the block order: plane-major, then tile row, then tile column
    m = torch.arange(2 * 17 * 65, dtype=F64).view(1, 2, 17, 65)
    s, cnt = R.tile_sums(m, 16, 64)
    assert cnt.tolist() == [1024, 16, 64, 1] * 2
    assert s[1] == m[0, 0, :16, 64].sum() and s[2] == m[0, 0, 16, :64].sum() and s[7] == m[0, 1, 16, 64]


def test_one_scale_loss_composes_to_msssim_autograd():
    """Two scales of msssim_ref under float64 autograd == one_scale_loss at scale 1 (SSIM mean), its gradient handed to scale 0
    as the coarse gradient next to scale 0's cs mean; and with w_sim = 1 it is ssim_ref's gradient."""
    for shape in ((2, 2, 23, 27), (1, 3, 30, 22)):
        a, b = (R.q32(t) for t in msssim_ref.textured_pair(shape, 0.3, 5))
        n = shape[0]
        g = torch.linspace(1.5, -0.5, n, dtype=F64) if n > 1 else torch.tensor([-0.75], dtype=F64)
        betas = msssim_ref.DEFAULT_BETAS[:2]
        x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
        val, v = msssim_ref.msssim_per_image(x, y, betas, None)
        (val * g).sum().backward()
        # the factors in float64 from the float64 values (combine() takes float32 raw values: not used here)
        bt = torch.tensor(betas, dtype=F64).view(-1, 1)
        f = bt * val.detach()[None] / v.detach()
        a1, b1 = TF.avg_pool2d(a, 2), TF.avg_pool2d(b, 2)
        c1a, c1b = R.one_scale_grads(a1, b1, 3, g, w_sim=f[1])
        g0a, g0b = R.one_scale_grads(a, b, 3, g, w_cs=f[0], coarse_a=c1a, coarse_b=c1b)
        for got, want in ((g0a, x.grad), (g0b, y.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
        (ssim_ref.ssim_per_image(x, y) * g).sum().backward()
        sa, sb = R.one_scale_grads(a, b, 3, g, w_sim=torch.ones(n, dtype=F64))
        assert float((sa - x.grad).abs().max()) <= 1e-12 and float((sb - y.grad).abs().max()) <= 1e-12
        # a dropped odd row / column gets nothing from the coarse term
        if shape[2] % 2 or shape[3] % 2:
            only = R.one_scale_grads(a, b, 1, g * 0, w_sim=f[1], coarse_a=c1a)[0]
            if shape[2] % 2:
                assert not bool(only[:, :, -1].any())
            if shape[3] % 2:
                assert not bool(only[:, :, :, -1].any())
            assert bool(only[:, :, 0, 0].any())


def test_psnr_reference_is_the_float64_formula():
    p, t = R.psnr_case(2, 32772)
    sse, keys = R.psnr_partials(p, t)
    pd, td = p.astype(np.float64), t.astype(np.float64)
    assert sse.sum() == ((pd - td) ** 2).sum() and len(sse) == 2 * 3
    for base, ls in zip((10.0, 2.0), R.LOG_SCALES):
        per = R.psnr_per_image(sse, 2, 32772, 2.5, ls)
        want = [10.0 * math.log(2.5 ** 2 / ((pd[i] - td[i]) ** 2).mean(), base) for i in range(2)]
        assert np.abs(per - want).max() <= 1e-6                          # log_scale is carried in float32: 6e-8 relative
        val, s, cnt, lo, hi = R.psnr_batch(sse, keys, 2, 32772, 1, 0.0, ls)
        assert (lo, hi) == (float(t.min()), float(t.max())) and cnt == 2 * 32772
        assert abs(val - 10.0 * math.log((max(hi, 0) - min(lo, 0)) ** 2 / ((pd - td) ** 2).mean(), base)) <= 1e-6
    st = R.psnr_state_after([0.0, 0.0, 0.0, 0.0], R.psnr_batch(sse, keys, 2, 32772, 1, 0.0, R.LOG_SCALES[0]))
    assert st == [sse.sum(), 2.0 * 32772, float(t.min()), float(t.max())]
    assert abs(R.psnr_of_state(st, 1, 0.0, R.LOG_SCALES[0]) - R.psnr_batch(sse, keys, 2, 32772, 1, 0.0, R.LOG_SCALES[0])[0]) <= 1e-12


def test_ordered_keys_follow_the_float_order():
    """Strictly increasing floats (with -0 below +0) give strictly increasing keys; unkey inverts key bit for bit."""
    vals = np.array([-np.inf, -3.4e38, -15.0, -3.0, -1.0, -2.0 ** -126, -1e-40, -(2.0 ** -149), -0.0, 0.0, 2.0 ** -149, 1e-40,
                     2.0 ** -126, 1.0, 7.0, 3.4e38, np.inf], dtype=np.float32)
    k = R.metric_key(vals)
    assert bool((k[1:] > k[:-1]).all()) and k.dtype == np.uint32
    assert np.array_equal(R.metric_unkey(k).view(np.uint32), vals.view(np.uint32))
    assert int(R.metric_key(np.float32(-0.0))) == 0x7FFFFFFF and int(R.metric_key(np.float32(0.0))) == 0x80000000
    assert set(R.SPECIALS.tolist()) <= set(vals.tolist()) and np.signbit(R.SPECIALS[0]) and not np.signbit(R.SPECIALS[1])
    # min / max over keys == min / max over floats on a table with every special
    _, t = R.psnr_case(2, 16388)
    ks = R.metric_key(t)
    assert float(R.metric_unkey(ks.min())) == float(t.min()) and float(R.metric_unkey(ks.max())) == float(t.max())


def test_combine_reference_is_msssim_ref():
    for normalize, name in ((0, None), (1, "relu"), (2, "simple")):
        a, b = (R.q32(t) for t in msssim_ref.textured_pair((3, 1, 50, 46), [0.05, 0.3, 1.0], 3))
        raw = msssim_ref.raw_scales(a, b, 3).numpy().astype(np.float32)
        betas = msssim_ref.DEFAULT_BETAS[:3]
        out, vals, fac = R.combine(raw, betas, normalize)
        r = torch.tensor(raw, dtype=F64, requires_grad=True)
        v = torch.relu(r) if normalize == 1 else (r + 1) / 2 if normalize == 2 else r
        bt = torch.tensor([R.f32(x) for x in betas], dtype=F64).view(-1, 1)
        want = torch.prod(v ** bt, dim=0)
        want.sum().backward()
        assert np.abs(out - want.detach().numpy()).max() <= 1e-6 and np.abs(fac - r.grad.numpy()).max() <= 1e-6
    # the stated rule under relu, and the plain arithmetic without it
    raw = np.array([[0.5, 0.0, -0.2, -0.0], [0.7, 0.6, 0.9, 0.8]], dtype=np.float32)
    out, vals, fac = R.combine(raw, (0.3, 0.7), 1)
    assert out[0] > 0 and out[1:].tolist() == [0.0, 0.0, 0.0] and not fac[:, 1:].any() and fac[:, 0].all()
    assert vals[0].tolist() == [0.5, 0.0, 0.0, 0.0]
    out, _, fac = R.combine(raw, (0.3, 0.7), 0)
    assert np.isnan(out[2]) and out[1] == 0.0 and np.isnan(fac[0, 1])


# ----------------------------------------------------------------------------- the exact regimes are exact
def test_identical_windows_give_exactly_one_in_float32():
    """ssim_of_moments / ssim_cs_of_moments restated in numpy float32 (one rounding per operation, nothing contracted): with
    identical windows (mb = ma, sbb = sab = saa) the value is exactly 1, whatever the moments' rounding -- and swapping the two
    images gives the same bits.  A sum of at most 1024 ones is exact, so an identical pair's partial is the tile's count."""
    rng = np.random.default_rng(0)
    f = np.float32
    ma = rng.uniform(0, 1.2, 20000).astype(f)
    saa = (ma * ma + rng.uniform(-1e-7, 0.1, 20000).astype(f)).astype(f)
    c1, c2 = f(R.C1), f(R.C2)

    def both(ma, mb, saa, sbb, sab):
        maa, mbb, mab = ma * ma, mb * mb, ma * mb
        va, vb, cab = saa - maa, sbb - mbb, sab - mab
        plain = ((f(2) * mab + c1) * (f(2) * cab + c2)) / ((maa + mbb + c1) * (va + vb + c2))
        cs = (f(2) * cab + c2) / (va + vb + c2)
        return plain, cs * ((f(2) * mab + c1) / (maa + mbb + c1)), cs

    for v in both(ma, ma, saa, saa, saa):
        assert v.dtype == np.float32 and bool((v == f(1)).all())
    mb = rng.uniform(0, 1.2, 20000).astype(f)
    sbb = (mb * mb + rng.uniform(0, 0.1, 20000).astype(f)).astype(f)
    sab = (ma * mb + rng.uniform(-0.05, 0.05, 20000).astype(f)).astype(f)
    for u, v in zip(both(ma, mb, saa, sbb, sab), both(mb, ma, sbb, saa, sab)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert R.SF_TH * R.SF_TW <= 2 ** 24


def test_psnr_cases_are_exact():
    for n, e, off in R.psnr_cases():
        if off:
            continue
        for shift in (0, -30, 40):
            if shift and (n, e) != (2, 32772):
                continue
            p, t = R.psnr_case(n, e, shift)
            d = p.astype(np.float64) - t.astype(np.float64)
            d32 = p - t                                                   # the kernel's float32 difference
            assert np.array_equal(d32.astype(np.float64), np.round(d)) and np.abs(d32).max() <= 15
            assert bool((d32[:, 0] != 0).all())
            sub = (t != 0) & (np.abs(t) < 2.0 ** -126)
            assert not d32[sub].any() and bool((np.round(d) == d)[~sub].all())
            sse, _ = R.psnr_partials(p, t)
            # every chunk's sum of |d|^2 stays below 2^24: any order of float32 additions and fmas is exact
            assert sse.max() <= 15 ** 2 * R.PSNR_CHUNK < 2 ** 24 and bool((sse == np.round(sse)).all())
            # the reference sums (p - t)^2 in float64; where t is subnormal p == t, so it is the same integer
            assert np.array_equal(sse.reshape(n, -1).sum(1), (d32.astype(np.float64) ** 2).sum(1))
            if e >= 3:
                assert np.signbit(t[n - 1][t[n - 1] == 0]).any() and (~np.signbit(t[n - 1][t[n - 1] == 0])).any()
            if e >= 16380:
                assert sub[n - 1].sum() >= 8 and (t[n - 1] == -15).any()
    assert 15 * 15 * 16384 == 3686400


def test_pool_and_accumulate_cases_are_exact():
    for planes, h, w, _ in R.POOL_CASES:
        x1, x2 = R.pool_case(planes, h, w)
        assert not torch.equal(x1, x2)
        for x in (x1, x2):
            assert torch.equal(x.to(F32).to(F64), x) and float(x.abs().max()) <= 64
            assert bool(((x * 16) == (x * 16).round()).all())
            ref = R.pool_ref(x)
            assert tuple(ref.shape) == (planes, h // 2, w // 2) and torch.equal(ref.to(F32).to(F64), ref)
            # float32 in the kernel's order
            y = x.to(F32)
            k = 0.25 * ((y[:, 0:h - h % 2:2, 0:w - w % 2:2] + y[:, 0:h - h % 2:2, 1::2][:, :, :w // 2])
                        + (y[:, 1::2, 0:w - w % 2:2][:, :h // 2] + y[:, 1::2, 1::2][:, :h // 2, :w // 2]))
            assert torch.equal(k.to(F64), ref)
    for n in R.ACC_N:
        v = R.acc_case(n).astype(np.float64)
        assert np.array_equal(v * 1024, np.round(v * 1024)) and np.abs(v).sum() < 2 ** 40
        assert float(np.sum(v)) == math.fsum(v)


# ----------------------------------------------------------------------------- the tables reach every branch
def test_case_tables_reach_every_branch():
    src = _flat_src()
    for line in (f"#defineSSIM_K{R.SSIM_K}", f"#defineSF_TW{R.SF_TW}", f"#defineSF_TH{R.SF_TH}",
                 f"#defineSB_T{R.SB_T}", f"#definePSNR_CHUNK{R.PSNR_CHUNK}",
                 "constintnm=(want_a&&want_b)?4:3;",
                 "constboolv4=E%4==0&&((uintptr_t)preds&15)==0&&((uintptr_t)target&15)==0;",
                 "constboolv4=W%4==0&&(((uintptr_t)in1|(uintptr_t)in2)&15)==0&&(((uintptr_t)out1|(uintptr_t)out2)&7)==0;"):
        assert line in src, line
    # the finalisers: images stride 16 waves, an image's blocks stride 64 lanes (three kernels); combine 256; accumulate 64
    assert src.count(f"for(intn=wave;n<N;n+={R.FIN_WAVES})") == 3
    assert src.count(f"for(intk=lane;k<nblk;k+={R.FIN_LANES})") == 2 and src.count(f"for(intk=lane;k<B;k+={R.FIN_LANES})") == 1
    assert f"for(intn=threadIdx.x;n<N;n+={R.COMBINE_THREADS})" in src and f"for(intn=threadIdx.x;n<N;n+={R.ACC_LANES})" in src
    # forward tiles: 1 position, 1 column, 1 row, full; blocks per image on both sides of the lane stride; N of the wave stride
    shapes, th, tw = R.FWD_SHAPES, R.SF_TH, R.SF_TW
    kinds = set()
    for shape in shapes:
        _, _, h, w = shape
        oh, ow = h - 10, w - 10
        ty, tx = R.tile_grid(oh, ow, th, tw)
        for iy in range(ty):
            for ix in range(tx):
                kinds.add((min(th, oh - iy * th), min(tw, ow - ix * tw)))
    assert {(1, 1), (th, 1), (1, tw), (th, tw)} <= kinds, kinds
    nblk = {R.blocks_per_image(s, R.SF_TH, R.SF_TW) for s in R.FWD_SHAPES}
    assert min(nblk) == 1 and max(nblk) > R.FIN_LANES and any(1 < b <= R.FIN_LANES for b in nblk)
    ns = {s[0] for s in R.FWD_SHAPES}
    assert min(ns) == 1 and any(R.FIN_WAVES < n for n in ns) and any(n > 4 * R.FIN_WAVES - 1 for n in ns)
    assert any(len(R.impulse_pixels(s, R.SF_TH, R.SF_TW)) == 6 for s in R.FWD_SHAPES)
    # backward: tile 32 with 32k + 1, a W in 33..42 (the tile's right halo leaves the image at once), nm 3 and 4, odd H and W
    hs, ws = {s[2] for s in R.BWD_SHAPES}, {s[3] for s in R.BWD_SHAPES}
    assert any(v % R.SB_T == 1 for v in hs | ws) and any(R.SB_T < w <= R.SB_T + 10 for w in hs | ws) and 11 in hs
    assert any(v % R.SB_T == 0 for v in hs) and {R.bwd_nm(w) for w in R.WHICH} == {3, 4}
    assert any(s[2] % 2 and s[3] % 2 for s in R.BWD_SHAPES) and any(s[0] > 1 for s in R.BWD_SHAPES)
    assert any(len(R.bwd_impulse_pixels(s)) == 6 for s in R.BWD_SHAPES)
    gs = torch.cat([R.bwd_case(s)[2] for s in R.BWD_SHAPES])
    assert bool((gs > 0).any()) and bool((gs < 0).any())
    for s in R.BWD_SHAPES:
        if s[0] > 1:
            g = R.bwd_case(s)[2]
            assert len(set(g.tolist())) == s[0] and bool((g > 0).any()) and bool((g < 0).any())
    combos = {(wh, wt, co) for _, wh, wt, co in R.ms_cases()}
    assert len(combos) == 3 * 3 * 2 + 3 and len(R.ms_cases()) == 21 * len(R.BWD_SHAPES)
    one = [R.bwd_args(s, 3, "both", "one") for s in R.BWD_SHAPES]
    assert any(a[5] is None and a[6] is not None for a in one) and any(a[5] is not None and a[6] is None for a in one)
    # PSNR: both forms (the scalar one two ways), the chunk edge on both sides, more than 64 chunks, N on both sides of 16
    cases = R.psnr_cases()
    assert {e for _, e, _ in cases} == set(R.PSNR_E) and {n for n, _, _ in cases} == set(R.PSNR_N)
    forms = {(R.psnr_form(e, off), e % 4 == 0) for _, e, off in cases}
    assert forms == {("v4", True), ("scalar", False), ("scalar", True)}
    assert {R.PSNR_CHUNK - 1, R.PSNR_CHUNK, R.PSNR_CHUNK + 1} <= set(R.PSNR_E)
    assert any(-(-e // R.PSNR_CHUNK) > R.FIN_LANES for _, e, _ in cases)
    assert any(n > R.FIN_WAVES and e > R.PSNR_CHUNK for n, e, _ in cases) and any(n > 2 * R.FIN_WAVES for n, _, _ in cases)
    assert all(n * e <= R.PSNR_MAX_ELEMENTS for n, e, _ in cases)
    assert {n // R.ACC_LANES for n in R.ACC_N} == {0, 1, 2} and R.ACC_LANES in R.ACC_N
    # pool: both forms, the scalar one by width and by alignment; odd H under V4; more than one block
    pf = {(R.pool_form(w, off), w % 4 == 0) for _, _, w, off in R.POOL_CASES}
    assert pf == {("v4", True), ("scalar", False), ("scalar", True)}
    assert any(h % 2 and R.pool_form(w, off) == "v4" for _, h, w, off in R.POOL_CASES)
    assert any(p * (h // 2) * (w // 4) > 256 for p, h, w, _ in R.POOL_CASES)
    # combine: N around the thread stride, L from 1 to the maximum
    assert {R.COMBINE_THREADS - 1, R.COMBINE_THREADS, R.COMBINE_THREADS + 1} <= set(R.COMBINE_N) and max(R.COMBINE_N) > 2 * R.COMBINE_THREADS
    assert min(R.COMBINE_L) == 1 and max(R.COMBINE_L) == len(R.BETAS8) == 8
    for n in R.COMBINE_N:
        for L in R.COMBINE_L:
            raw = R.combine_case(n, L)
            assert raw.shape == (L, n) and raw.min() > -0.61 and raw.max() <= 1.0
            if n > 1:
                z = raw[raw == 0]
                assert (raw < 0).any() and np.signbit(z).any() and (~np.signbit(z)).any() and bool((raw[:, 0] > 0).all())


# ----------------------------------------------------------------------------- the floors of the measured bars
def test_forward_floors():
    """F(n) of the forward tile, printed; the bar is 4 x max(F(n), 1e-6 n).  A wrong mask (one position more or less in a tile)
    moves a sum by about one SSIM value, 0.1 .. 1: far above every bar of a tile that can hold such an error."""
    th, tw, shapes = R.SF_TH, R.SF_TW, R.FWD_SHAPES
    fl = R.fwd_floor(th, tw)
    print(f"\nforward floors, tile {th} x {tw}: " + ", ".join(f"F({n}) = {f:.3e} ({f / n:.2e}/pos)" for n, f in sorted(fl.items())))
    for n, f in fl.items():
        assert 0.0 <= f <= 2e-5 * n, (n, f)
        assert float(R.fwd_bar(np.array([n]), th, tw)[0]) <= 0.1
    assert {1, th, tw, th * tw} <= set(fl)
    for shape in shapes:
        assert set(R.tile_counts(shape, th, tw).tolist()) <= set(fl)


def test_backward_floors():
    """The float32 CPU floors of both gradient bars over the whole table (plain and multi-scale, impulse inputs), printed."""
    worst = {}
    for shape in R.BWD_SHAPES:
        for which in R.WHICH:
            rows = [("plain", R.bwd_reference(shape, which, None, "none"))]
            rows += [("ms", R.bwd_reference(shape, which, wt, co)) for s, wh, wt, co in R.ms_cases() if s == shape and wh == which]
            for kind, refs in rows:
                for r in refs:
                    if r is not None:
                        w = worst.setdefault(kind, [0.0, 0.0])
                        w[0], w[1] = max(w[0], r[1]), max(w[1], r[2])
                        assert r[1] < 1e-4 and r[2] < 1e-4 and float(r[0].abs().max()) > 0
        for y, x in R.bwd_impulse_pixels(shape):
            for kind, wt in (("plain impulse", None), ("ms impulse", "both")):
                kind += " (image corner)" if (y, x) in ((0, 0), (shape[2] - 1, shape[3] - 1)) else " (tile corner)"
                refs = R.bwd_reference(shape, 3, wt, "none", (y, x))
                far = R.far_from_impulse(shape, y, x)
                for r in refs:
                    w = worst.setdefault(kind, [0.0, 0.0])
                    w[0], w[1] = max(w[0], r[1]), max(w[1], r[2])
                    # the gradient is that of one pixel's windows while float32's rounding noise covers the plane: the floor is
                    # percent-sized for an interior pixel and above 1 for a corner pixel, which a single window position
                    # reaches with weight g[0]^2 = 1e-6; so is the bar.  What these cases add is the localisation.
                    assert math.isfinite(r[1]) and math.isfinite(r[2])
                    if (y, x) not in ((0, 0), (shape[2] - 1, shape[3] - 1)):
                        assert r[1] < 0.1 and r[2] < 0.1
                    # float64: zero away from the impulse (to rounding), so the bar there is the per-pixel bar alone
                    if bool(far.any()):
                        assert float(r[0][far].abs().max()) <= 1e-15
    for kind, (l2, mx) in worst.items():
        bl, bm = R.bwd_bars(l2, mx)
        print(f"\nbackward floors, {kind}: rel L2 {l2:.3e} (bar up to {bl:.3e}), per pixel / max|ref| {mx:.3e} (bar up to {bm:.3e})")
