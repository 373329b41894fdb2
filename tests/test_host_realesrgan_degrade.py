"""CPU: the host side of the second-order Real-ESRGAN degradation -- the kernel family, the Bessel function behind the sinc
filter, the torch-convention resize tables against F.interpolate in float64, the pair pool, the degradation plan, and the
no-GPU errors of the new ops."""
import importlib
import math

import numpy as np
import pytest
import torch

import interpolate_ref as IR

PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


# ----------------------------------------------------------------------------- kernels
def test_kernels_sum_to_one():
    D = P("utils.degradation")
    ks = [D.generalized_gaussian_kernel(21, 2.0, 0.7, 0.6, 0.5), D.generalized_gaussian_kernel(7, 0.2, 0.2, 0.0, 3.9),
          D.plateau_kernel(21, 3.0, 0.4, -1.0, 1.7), D.plateau_kernel(9, 1.0, 1.0, 0.0, 1.0),
          D.sinc_kernel(math.pi / 3, 7), D.sinc_kernel(math.pi / 5, 21), D.sinc_kernel(3.0, 13, pad_to=21)]
    ks += list(D.random_mixed_kernels(24, size=tuple(range(7, 22, 2)), sinc_prob=0.3, rng=np.random.RandomState(3)))
    for k in ks:
        assert k.dtype == np.float32 and k.shape[0] == k.shape[1]
        assert abs(float(k.sum(dtype=np.float32)) - 1.0) < 1e-6


def test_generalized_beta_one_is_the_gaussian_bit_for_bit():
    D = P("utils.degradation")
    for size, sx, sy, th in ((21, 2.3, 0.9, 0.7), (7, 0.2, 0.2, 0.0), (13, 3.0, 1.1, -2.0)):
        assert np.array_equal(D.generalized_gaussian_kernel(size, sx, sy, th, 1.0), D.gaussian_kernel(size, sx, sy, th))
        assert np.array_equal(D.generalized_gaussian_kernel(size, sx, sy, th, 1), D.gaussian_kernel(size, sx, sy, th))


def test_sinc_kernel_symmetry_padding_and_centre():
    D = P("utils.degradation")
    k = D.sinc_kernel(1.9, 15)
    for m in (k.T, k[::-1], k[:, ::-1], k[::-1, ::-1], k.T[::-1], k.T[:, ::-1], k.T[::-1, ::-1]):
        assert np.array_equal(k, m)
    p = D.sinc_kernel(1.9, 15, pad_to=21)
    assert p.shape == (21, 21) and np.array_equal(p[3:18, 3:18], k) and p.sum(dtype=np.float64) == k.sum(dtype=np.float64)
    # the centre tap is cutoff^2 / (4 pi): its ratio to a neighbour is that of the formula
    c = 1.9
    want = (c * c / (4 * math.pi)) / (c * float(D.bessel_j1(c)) / (2 * math.pi))
    assert abs(float(k[7, 7]) / float(k[7, 8]) - want) < 1e-6


def test_bessel_j1():
    D = P("utils.degradation")
    assert abs(float(D.bessel_j1(1.0)) - 0.44005058574493355) < 1e-14
    assert abs(float(D.bessel_j1(10.0)) - 0.04347274616886141) < 1e-14
    assert float(D.bessel_j1(0.0)) == pytest.approx(0.0, abs=1e-16)


def test_sinc_kernel_against_scipy():
    special = pytest.importorskip("scipy.special")
    D = P("utils.degradation")
    for cutoff, size in ((math.pi / 5, 21), (2.5, 7), (math.pi - 1e-3, 21)):
        r = size // 2
        y, x = np.meshgrid(np.arange(size) - r, np.arange(size) - r, indexing="ij")
        rho = np.hypot(x, y).astype(np.float64)
        rho[r, r] = 1.0
        k = cutoff * special.j1(cutoff * rho) / (2 * math.pi * rho)
        k[r, r] = cutoff * cutoff / (4 * math.pi)
        k /= k.sum()
        assert np.abs(D.sinc_kernel64(cutoff, size) - k).max() < 1e-12            # the float64 stage; sinc_kernel rounds it once
        assert np.array_equal(D.sinc_kernel(cutoff, size), D.sinc_kernel64(cutoff, size).astype(np.float32))
    xs = np.linspace(0.0, 45.0, 4001)
    assert np.abs(D.bessel_j1(xs) - special.j1(xs)).max() < 1e-12


def test_random_mixed_kernels_repeat_and_cover():
    D = P("utils.degradation")
    kw = dict(size=tuple(range(7, 22, 2)), sigma_x=(0.2, 3.0), sigma_y=(0.2, 3.0), betag=(0.5, 4.0), betap=(1.0, 2.0), sinc_prob=0.1)
    a = D.random_mixed_kernels(64, rng=np.random.RandomState(11), **kw)
    b = D.random_mixed_kernels(64, rng=np.random.RandomState(11), **kw)
    assert a.shape == (64, 21, 21) and a.dtype == np.float32 and np.array_equal(a, b)
    assert not np.array_equal(a, D.random_mixed_kernels(64, rng=np.random.RandomState(12), **kw))
    supports = {int((np.abs(k).sum(axis=0) > 0).sum()) for k in a}
    assert len(supports) > 3 and min(supports) >= 7 and max(supports) == 21          # several sizes, padded symmetrically
    for k in a:
        on = np.nonzero(np.abs(k).sum(axis=0) > 0)[0]
        assert on[0] == 20 - on[-1]
    assert (a < 0).any()                                                               # a sinc kernel was drawn
    with pytest.raises(ValueError):
        D.random_mixed_kernels(1, kernel_list=("iso", "box"), kernel_prob=(0.5, 0.5))
    with pytest.raises(ValueError):
        D.random_mixed_kernels(1, size=8)


# ----------------------------------------------------------------------------- interpolate tables
def _host_tables(I, n_in, n_out, mode, sf):
    w, idx = I.interpolate_axis_weights(n_in, n_out, mode, sf)
    return w, idx


@pytest.mark.parametrize("mode", IR.MODES)
def test_interpolate_tables_equal_torch_in_float64(mode):
    I = P("utils.imresize")
    rs = np.random.RandomState(0)
    worst = 0.0
    for h, w in IR.SIZES:
        x = rs.rand(1, 2, h, w)
        for s in IR.SCALES:
            for form in ("scale_factor", "size"):
                if form == "scale_factor":
                    oh, ow = IR.out_size(h, scale_factor=s), IR.out_size(w, scale_factor=s)
                    want = IR.torch_interpolate(x, scale_factor=s, mode=mode).numpy()
                    th, tw = _host_tables(I, h, oh, mode, s), _host_tables(I, w, ow, mode, s)
                    loop = IR.loop_interpolate(x, scale_factor=s, mode=mode)
                else:
                    oh, ow = max(1, int(round(h * s)) + 1), max(1, int(round(w * s)) + 2)
                    want = IR.torch_interpolate(x, size=(oh, ow), mode=mode).numpy()
                    th, tw = _host_tables(I, h, oh, mode, None), _host_tables(I, w, ow, mode, None)
                    loop = IR.loop_interpolate(x, size=(oh, ow), mode=mode)
                assert I.interpolate_out_size(h, scale_factor=s) == IR.out_size(h, scale_factor=s)
                got = IR.apply_tables(x, th, tw)
                assert got.shape == want.shape == (1, 2, oh, ow)
                worst = max(worst, np.abs(got - want).max(), np.abs(loop - want).max())
    assert worst < 1e-13, worst


def test_interpolate_tables_layout_and_transpose():
    I = P("utils.imresize")
    for mode, n_in, n_out, sf in (("area", 40, 6, 0.15), ("bilinear", 17, 25, 1.5), ("bicubic", 23, 11, None), ("area", 33, 33, 1.0)):
        t = I.interpolate_tables(n_in, n_out, mode, sf, device="cpu")
        assert t is I.interpolate_tables(n_in, n_out, mode, sf, device="cpu")        # cached per argument tuple
        assert (t.n_in, t.n_out) == (n_in, n_out) and t.idx.dtype == torch.int32 and t.w.dtype == torch.float32
        assert tuple(t.idx.shape) == tuple(t.w.shape) == (n_out, t.taps) and t.taps <= 9
        assert int(t.idx.min()) >= 0 and int(t.idx.max()) < n_in
        fwd = np.zeros((n_out, n_in), dtype=np.float64)
        for o in range(n_out):
            for k in range(t.taps):
                fwd[o, int(t.idx[o, k])] += float(t.w[o, k])
        bwd = np.zeros((n_in, n_out), dtype=np.float64)
        for i in range(n_in):
            for k in range(t.q):
                bwd[i, int(t.t_idx[i, k])] += float(t.t_w[i, k])
        assert np.abs(fwd.T - bwd).max() < 1e-7
        assert np.abs(fwd.sum(axis=1) - 1.0).max() < 1e-6
    with pytest.raises(ValueError):
        I.interpolate_tables(8, 4, "nearest", None, device="cpu")


# ----------------------------------------------------------------------------- pair pool
def test_pair_pool_on_cpu_tensors():
    R = P("utils.realesrgan")
    pool = R.PairPool(size=6, seed=1)
    nxt = [0]

    def batch():
        ids = torch.arange(nxt[0], nxt[0] + 2, dtype=torch.float32)
        nxt[0] += 2
        return ids.reshape(2, 1, 1, 1).expand(2, 3, 2, 2).clone(), (ids + 0.5).reshape(2, 1, 1, 1).expand(2, 3, 4, 4).clone()

    for _ in range(3):                                     # until full: returns its input
        lq, gt = batch()
        out_lq, out_gt = pool(lq, gt)
        assert torch.equal(out_lq, lq) and torch.equal(out_gt, gt)
    moved = False
    for _ in range(5):
        before = sorted(pool.lq[:, 0, 0, 0].tolist())
        lq, gt = batch()
        out_lq, out_gt = pool(lq, gt)
        after = sorted(pool.lq[:, 0, 0, 0].tolist())
        ids_in, ids_out = lq[:, 0, 0, 0].tolist(), out_lq[:, 0, 0, 0].tolist()
        assert sorted(after + ids_out) == sorted(before + ids_in)                     # the multiset is kept
        assert torch.equal(out_gt[:, 0, 0, 0], out_lq[:, 0, 0, 0] + 0.5)               # pairs stay together
        assert torch.equal(pool.gt[:, 0, 0, 0], pool.lq[:, 0, 0, 0] + 0.5)
        assert torch.equal(pool.lq[:2], lq)
        moved = moved or ids_out != ids_in
    assert moved
    a, b = R.PairPool(size=4, seed=7), R.PairPool(size=4, seed=7)                      # the same seed repeats
    for _ in range(6):
        lq, gt = batch()
        assert torch.equal(a(lq, gt)[0], b(lq, gt)[0])
    with pytest.raises(ValueError):
        R.PairPool(size=5)(*batch())


# ----------------------------------------------------------------------------- the plan
def test_degradation_plan_repeats_and_stays_in_range():
    R = P("utils.realesrgan")
    deg = R.RealESRGANDegradation(scale=4)
    seen = set()
    for seed in range(40):
        p = deg.plan(3, 128, 96, np.random.RandomState(seed))
        q = deg.plan(3, 128, 96, np.random.RandomState(seed))
        for name, v in p.__dict__.items():
            w = q.__dict__[name]
            assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w, name
        for k in (p.kernel1, p.kernel2, p.sinc_kernel):
            assert k.shape == (3, 21, 21) and k.dtype == np.float32
            assert np.abs(k.sum(axis=(1, 2), dtype=np.float64) - 1.0).max() < 1e-6
        assert 0.15 <= p.scale1 <= 1.5 and 0.3 <= p.scale2 <= 1.2
        assert {p.mode1, p.mode2, p.mode3} <= set(R.RESIZE_MODES) and p.noise1 in ("gaussian", "poisson") and p.noise2 in ("gaussian", "poisson")
        lo1, hi1 = (1, 30) if p.noise1 == "gaussian" else (0.05, 3)
        lo2, hi2 = (1, 25) if p.noise2 == "gaussian" else (0.05, 2.5)
        assert p.amount1.shape == p.amount2.shape == (3,) and p.amount1.dtype == np.float32
        assert (p.amount1 >= lo1).all() and (p.amount1 <= hi1).all() and (p.amount2 >= lo2).all() and (p.amount2 <= hi2).all()
        assert p.gray1.shape == p.gray2.shape == (3,) and p.gray1.dtype == np.bool_
        for qv in (p.quality1, p.quality2):
            assert qv.shape == (3,) and qv.dtype == np.int32 and qv.min() >= 30 and qv.max() <= 95
        assert p.size1 == (int(math.floor(128 * p.scale1)), int(math.floor(96 * p.scale1)))
        assert p.size2 == (int(128 / 4 * p.scale2), int(96 / 4 * p.scale2)) and p.size3 == (32, 24)
        assert min(p.size1) >= 11
        seen.add((p.second_blur, p.jpeg_last, p.noise1))
    assert len(seen) >= 6                                                              # the branches are all drawn
    with pytest.raises(ValueError):
        deg.plan(2, 40, 40)                                                            # 10 output pixels: no room for the filters
    with pytest.raises(ValueError):
        deg.plan(2, 66, 64)


# ----------------------------------------------------------------------------- argument checks run on the host
def test_new_entry_points_check_their_arguments_before_launching():
    import ctypes
    lib = P("_lib").lib()
    N, st = None, None
    a, b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)          # never dereferenced: validation fails first
    calls = [
        lambda: lib.dsr_filter2d_f32(N, b, a, 1, 3, 32, 32, 21, 0, st),
        lambda: lib.dsr_filter2d_f32(a, N, a, 1, 3, 32, 32, 21, 0, st),
        lambda: lib.dsr_filter2d_f32(a, b, N, 1, 3, 32, 32, 21, 0, st),
        lambda: lib.dsr_filter2d_f32(a, b, a, 0, 3, 32, 32, 21, 0, st),
        lambda: lib.dsr_filter2d_f32(a, b, a, 1, 3, 10, 32, 21, 0, st),          # H = 10 cannot reflect 10 rows
        lambda: lib.dsr_filter2d_f32(a, b, a, 1, 3, 32, 10, 21, 0, st),
        lambda: lib.dsr_filter2d_f32(a, b, a, 1, 3, 32, 32, 8, 0, st),           # even
        lambda: lib.dsr_filter2d_f32(a, b, a, 1, 3, 32, 32, 23, 0, st),          # > 21
        lambda: lib.dsr_filter2d_f32(a, a, a, 1, 3, 32, 32, 21, 0, st),          # y == x
        lambda: lib.dsr_filter2d_f32(a, ctypes.c_void_p((1 << 20) + 64), a, 1, 3, 32, 32, 21, 0, st),      # y inside x
        lambda: lib.dsr_filter2d_f32(a, b, a, 1, 3, 32, 32, 21, 2, st),          # shared flag
        lambda: lib.dsr_filter2d_f32(a, b, a, 8, 4, 8192, 8192, 21, 0, st),      # 2^31 elements
        lambda: lib.dsr_noise_gaussian_f32(N, a, a, a, a, a, 1, 8, 8, st),
        lambda: lib.dsr_noise_gaussian_f32(a, a, a, a, N, a, 1, 8, 8, st),
        lambda: lib.dsr_noise_gaussian_f32(a, a, a, a, a, a, 1, 0, 8, st),
        lambda: lib.dsr_noise_gaussian_f32(a, a, a, a, a, a, 3, 16384, 16384, st),
        lambda: lib.dsr_noise_poisson_f32(a, a, a, N, a, a, a, 1, 8, 8, st),
        lambda: lib.dsr_noise_poisson_f32(a, a, a, a, a, a, N, 1, 8, 8, st),
        lambda: lib.dsr_noise_poisson_f32(a, a, a, a, a, a, a, 0, 8, 8, st),
        lambda: lib.dsr_usm_mask(a, N, 10.0, a, 64, st),
        lambda: lib.dsr_usm_mask(a, a, 10.0, a, 0, st),
        lambda: lib.dsr_usm_combine(a, a, N, 0.5, a, 64, st),
        lambda: lib.dsr_usm_combine(a, a, a, 0.5, a, 1 << 31, st),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert lib.dsr_last_error(), i


# ----------------------------------------------------------------------------- no GPU, no result
def test_new_ops_refuse_cpu_tensors():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    D, I, R = P("utils.degradation"), P("utils.imresize"), P("utils.realesrgan")
    x = torch.rand(2, 3, 32, 32)
    k = torch.from_numpy(D.random_mixed_kernels(2, rng=np.random.RandomState(0)))
    calls = [lambda: D.filter2d(x, k), lambda: I.interpolate(x, scale_factor=0.5, mode="area"),
             lambda: I.interpolate(x, size=(8, 8), mode="bicubic"),
             lambda: D.add_gaussian_noise_batch(x, 10.0, False), lambda: D.add_poisson_noise_batch(x, 1.0, True),
             lambda: D.usm_sharp(x), lambda: D.USMSharp()(x), lambda: R.RealESRGANDegradation(scale=2)(x)]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    with pytest.raises(ValueError):
        D.usm_sharp(torch.rand(1, 3, 25, 40))
    with pytest.raises(ValueError):
        D.usm_sharp(torch.rand(1, 1, 40, 25))
