"""CPU: the resampling sweep's reference and case tables (tests/resample_ref.py) against float64 torch.

Nothing here launches a kernel.  Each index-level restatement is pinned to the torch op it restates, forward and (through
autograd) backward, NaN / tie / infinity windows of the max pool included; every exact-regime table entry is shown to be
representable in bf16 and in fp16, outputs and gradients; the hand-built resize tables are shown to hold the window counts
the GPU sweep relies on; and the argument checks that fail before any launch are made here as well."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import resample_ref as R

PKG = "deep-super-resolution_amd"


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def same(got, want, what):
    """Equality with NaN == NaN and -0 == +0."""
    assert got.shape == want.shape, what
    bad = (got != want) & ~(got.isnan() & want.isnan())
    assert not bool(bad.any()), (what, bad.nonzero()[:4].tolist())


def close(got, want, what):
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), what


def grad_of(fn, x, dy):
    """float64 autograd gradient of fn at NHWC x for the NHWC output gradient dy."""
    z = nchw(x).clone().requires_grad_(True)
    fn(z).backward(nchw(dy))
    return nhwc(z.grad)


# ----------------------------------------------------------------------------- the reference is the contract
@pytest.mark.parametrize("windows", [R.MAXPOOL_EDGES, R.RELU_EDGES], ids=["edges", "relu_edges"])
def test_maxpool_reference_on_edge_windows(windows):
    """NaN at each position and in pairs, +-Inf, all-equal windows and pairwise ties, odd H and W: value and gradient routing
    of the reference are nn.MaxPool2d's in float64 (a NaN propagates, the last NaN of a window takes the gradient, otherwise
    the first maximum; an Inf / NaN gradient reaches one input)."""
    x, dy = R.edge_case(windows)
    pool = lambda z: TF.max_pool2d(z, 2, 2)
    same(R.maxpool2_fwd(x), nhwc(pool(nchw(x))), "forward")
    dx = R.maxpool2_bwd(x, dy)
    same(dx, grad_of(pool, x, dy), "backward")
    assert float(dx[:, 2].abs().sum()) == 0.0 and float(dx[:, :, -1].abs().sum()) == 0.0      # trailing row / column
    hits = (dx != 0) | dx.isnan()
    assert int(hits.sum()) == int(((dy != 0) | dy.isnan()).sum())                              # each dy reaches ONE input
    # every window of the table really has the winner the issue's rule names (independent of torch)
    for win in windows:
        m, arg = win[0], 0
        for q in (1, 2, 3):
            if win[q] > m or win[q] != win[q]:
                m, arg = win[q], q
        xm, xarg = R.maxpool2_scan(torch.tensor(win, dtype=torch.float64).reshape(1, 2, 2, 1))
        assert int(xarg) == arg and (float(xm) == m or (m != m and bool(xm.isnan())))


def test_maxpool_relu_masked_reference():
    """The ReLU-masked backward == autograd through max_pool2d(relu(x)) for a ReLU output x (finite >= 0, or +Inf): an all-zero
    window gives 0, a +Inf maximum passes its gradient."""
    x, dy = R.edge_case(R.RELU_EDGES)
    dy = torch.where(dy.isfinite(), dy, torch.ones_like(dy))      # (0 * Inf of autograd's ReLU would be NaN where the kernel selects)
    want = grad_of(lambda z: TF.max_pool2d(torch.relu(z), 2, 2), x, dy)
    same(R.maxpool2_bwd(x, dy, relu_mask=True), want, "relu-masked backward")
    zero = R.RELU_EDGES.index((0, 0, 0, 0))
    inf = R.RELU_EDGES.index((R.INF, 1, 2, 3))
    got = R.maxpool2_bwd(x, dy, relu_mask=True)
    k = len(R.RELU_EDGES)
    for pos in range(k):
        win = (pos + 0 + 0) % k          # lane 0 of image 0
        if win == zero:
            assert float(got[0, :2, 2 * pos:2 * pos + 2, 0].abs().sum()) == 0.0
        if win == inf:
            assert float(got[0, 0, 2 * pos, 0]) == float(dy[0, 0, pos, 0]) != 0.0


@pytest.mark.parametrize("n,h,w,cp", R.shapes(thin=True), ids=lambda v: str(v))
def test_exact_cases_against_torch_and_representable(n, h, w, cp):
    """Every exact-regime case: the references equal float64 torch (values and autograd gradients), and every input, output and
    gradient round-trips through bf16 and through fp16, so that the GPU sweep may compare with equality."""
    d = R.exact_case(n, h, w, cp)
    up = lambda mode: (lambda z: TF.interpolate(z, scale_factor=2, mode=mode, **({"align_corners": False} if mode == "bilinear" else {})))
    close(d["bil_y"], nhwc(up("bilinear")(nchw(d["bil_x"]))), "bilinear forward")
    close(d["bil_dx"], grad_of(up("bilinear"), d["bil_x"], d["bil_dy"]), "bilinear backward")
    near = R.nearest2x_fwd(d["bil_x"])
    same(near, nhwc(up("nearest")(nchw(d["bil_x"]))), "nearest forward")
    close(d["near_dx"], grad_of(up("nearest"), d["bil_x"], d["near_dy"]), "nearest backward")
    # the adjoint identity <fwd(x), dy> == <x, bwd(dy)>, exact on the grids
    assert float((d["bil_y"] * d["bil_dy"]).sum()) == float((d["bil_x"] * d["bil_dx"]).sum())
    assert float(d["bil_y"].abs().max()) <= 48 and float(d["bil_dx"].abs().max()) <= 192
    keys = ["bil_x", "bil_dy", "bil_y", "bil_dx", "near_dy", "near_dx", "avg_x", "avg_dy", "avg_dx"]
    if h >= 2 and w >= 2:
        avg = lambda z: TF.avg_pool2d(z, 2, 2)
        pool = lambda z: TF.max_pool2d(z, 2, 2)
        close(d["avg_y"], nhwc(avg(nchw(d["avg_x"]))), "avgpool forward")
        close(d["avg_dx"], grad_of(avg, d["avg_x"], d["avg_dy"]), "avgpool backward")
        same(R.maxpool2_fwd(d["max_x"]), nhwc(pool(nchw(d["max_x"]))), "maxpool forward")
        same(d["max_dx"], grad_of(pool, d["max_x"], d["max_dy"]), "maxpool backward")
        same(d["relu_dx"], grad_of(lambda z: pool(torch.relu(z)), d["relu_x"], d["max_dy"]), "maxpool relu backward")
        keys += ["avg_y", "max_x", "max_dy", "max_dx", "relu_x", "relu_dx"]
    else:
        assert float(d["avg_dx"].abs().sum()) == 0.0            # H or W of 1: no window, the adjoint is all zero
    for key in keys:
        for dt in (R.BF16, R.F16):
            assert R.representable(d[key], dt), (key, dt)


def test_random_bit_patterns_pool_as_torch():
    """Max pool on arbitrary 16-bit patterns (NaNs, infinities, subnormals, signed zeros): the element the reference's scan ends
    on is torch's, for both storage types."""
    for dt in (R.BF16, R.F16):
        bits = R.bits16(R._gen(3, dt), (3, 7, 10, 24), dt)
        x = bits.view(R.DTYPES[dt]).to(torch.float64)
        assert bool(x.isnan().any()) and bool(x.isinf().any())
        m, arg = R.maxpool2_scan(x)
        same(m, nhwc(TF.max_pool2d(nchw(x), 2, 2)), "forward")
        picked = R.take_by_arg(bits, arg).view(R.DTYPES[dt]).to(torch.float64)
        same(picked, m, "the picked bit pattern is the maximum")


def test_fp16_finite_range_edges():
    """Four times 65504: the mean is 65504 (a 16-bit accumulation would overflow), the nearest adjoint's sum rounds to +Inf."""
    x = torch.full((1, 2, 2, 8), R.F16_MAX, dtype=torch.float64)
    assert float(R.r16(R.avgpool2_fwd(x)[0], R.F16).max()) == R.F16_MAX
    assert bool(R.r16(R.nearest2x_bwd(x)[0], R.F16).isinf().all())


# ----------------------------------------------------------------------------- resize + normalise
def _gan():
    return importlib.import_module(PKG + ".utils.GAN")


def test_resize_table_family():
    """The hand-built family: column counts 1, 15, 16, 17 and 40 (both sides of the kernel's nx <= 16 branch, its boundary, and
    more than 33), row counts 1 and 9, every window inside the image, the windows over 16 columns wide not at output 0 (where a
    wrong row stride of the weight table would not show) and every row of the weight table different."""
    wy, wx = R.resize_family()
    xc = [len(w) for _, w in wx]
    assert {1, 15, 16, 17} <= set(xc) and max(xc) >= 33 and set(len(w) for _, w in wy) == {1, 9}
    for wins, size in ((wy, R.RESIZE_H), (wx, R.RESIZE_W)):
        for s, w in wins:
            assert 0 <= s and s + len(w) <= size and w.dtype == np.float32 and abs(float(w.sum()) - 1) < 1e-6
    wide = [o for o, c in enumerate(xc) if c > 16]
    assert len(wide) >= 2 and min(wide) > 0
    for a in wide:
        for b in range(len(wx)):
            if a != b:
                n = min(xc[a], xc[b])
                assert not np.array_equal(wx[a][1][:n], wx[b][1][:n])
    n_fwd = 2 * len(wy) * len(wx)
    n_bwd = 2 * R.RESIZE_H * R.RESIZE_W
    assert n_fwd > 256 and n_fwd % 256 and n_bwd > 256 and n_bwd % 256


@pytest.mark.parametrize("c", [1, 3])
def test_resize_reference(c):
    """The table-driven reference: with identity tables it is (x - mean) / std; with the hand-built family it equals the plain
    triple loop at a few outputs; and with the transposed tables of utils.GAN._transpose_windows its backward is the adjoint
    of its forward in float64."""
    G = _gan()
    g = R._gen(5, c)
    h, w = R.RESIZE_H, R.RESIZE_W
    src = torch.randn(2, c, h, w, generator=g, dtype=torch.float64)
    mean, std = R.RESIZE_MEAN, R.RESIZE_STD
    iy, ix = R.pack_tables(R.identity_windows(h), 1), R.pack_tables(R.identity_windows(w), 1)
    out, _ = R.resize_norm_fwd(src, iy, ix, mean, std)
    want = (src - R._chan(mean, c).reshape(1, c, 1, 1)) / R._chan(std, c).reshape(1, c, 1, 1)
    close(out[..., :c], nhwc(want), "identity")
    assert float(out[..., c:].abs().sum()) == 0.0
    wy, wx = R.resize_family()
    ty, tx = G._transpose_windows(wy, h), G._transpose_windows(wx, w)
    kt = max(max(len(v) for _, v in t) for t in (wy, wx, ty, tx))
    out, a = R.resize_norm_fwd(src, R.pack_tables(wy, kt), R.pack_tables(wx, kt), mean, std)
    for oy, ox in ((0, 0), (3, 4), (9, 14), (4, 9)):
        for ch in range(c):
            acc = 0.0
            for i, vy in enumerate(wy[oy][1]):
                for j, vx in enumerate(wx[ox][1]):
                    acc += float(vy) * float(vx) * float(src[1, ch, wy[oy][0] + i, wx[ox][0] + j])
            want = (acc - float(np.float32(mean[ch]))) / float(np.float32(std[ch]))
            assert abs(float(out[1, oy, ox, ch]) - want) <= 1e-12 * float(a[1, oy, ox, ch])
    dout = torch.randn(2, len(wy), len(wx), 8, generator=g, dtype=torch.float64)
    dsrc, _ = R.resize_norm_bwd(dout, R.pack_tables(ty, kt), R.pack_tables(tx, kt), std, c, h, w)
    lin = out[..., :c] + (R._chan(mean, c) / R._chan(std, c))            # the linear part of the forward
    lhs, rhs = float((lin * dout[..., :c]).sum()), float((src * dsrc).sum())
    assert abs(lhs - rhs) <= 1e-10 * float((a[..., :c] * dout[..., :c].abs()).sum())


def test_product_tables_reach_the_generic_loop():
    """ResampleTables(144, 160, resize_to=16, crop=12), a 9x downscale: its column windows are wider than the 16 the register
    path of resize_norm_fwd_kernel holds."""
    tab = _gan().ResampleTables(144, 160, "cpu", resize_to=16, crop=12)
    assert (tab.out_h, tab.out_w) == (12, 12)
    assert int(tab.xc.max()) > 16 and int(tab.yc.max()) > 16


# ----------------------------------------------------------------------------- downsampler
def _ds_torch(x, kern, f, p):
    nc = x.shape[0]
    z = TF.pad(x[None], (p, p, p, p), mode="replicate") if p else x[None]
    return TF.conv2d(z, kern[None, None].repeat(nc, 1, 1, 1), stride=f, groups=nc)[0]


def test_downsampler_cases_cover_the_edges():
    cases = R.ds_cases()
    assert {c[0] for c in cases} == set(R.DS_K) and {c[1] for c in cases} == set(R.DS_F)
    assert any(h == 1 and p > 0 for k, f, p, h, w in cases)                      # both replicate ends fold onto one row
    assert any(p >= h and h > 1 for k, f, p, h, w in cases)
    assert any((h + 2 * p - k) % f and (w + 2 * p - k) % f for k, f, p, h, w in cases)
    assert any(R.DS_NC * h * w > 256 and (R.DS_NC * h * w) % 256 for k, f, p, h, w in cases)
    assert any(R.DS_NC * R.ds_out(h, k, f, p) * R.ds_out(w, k, f, p) > 256 for k, f, p, h, w in cases)
    for k in R.DS_K:
        kern = R.ds_kernel(k)
        assert not torch.equal(kern, kern.t())
    for k, f, p, h, w in R.DS_EMPTY:
        assert R.ds_out(h, k, f, p) == 0 or R.ds_out(w, k, f, p) == 0
    assert any(-f < h + 2 * p - k < 0 or -f < w + 2 * p - k < 0 for k, f, p, h, w in R.DS_EMPTY)


@pytest.mark.parametrize("k", R.DS_K)
def test_downsampler_reference(k):
    """Forward == replicate pad + strided depthwise conv2d in float64; backward == its autograd gradient; for every case."""
    kern = R.ds_kernel(k)
    for kk, f, p, h, w in R.ds_cases():
        if kk != k:
            continue
        g = R._gen(11, k, f, p, h, w)
        x = torch.randn(R.DS_NC, h, w, generator=g, dtype=torch.float64)
        y, a = R.downsample_fwd(x, kern, f, p)
        z = x.clone().requires_grad_(True)
        want = _ds_torch(z, kern, f, p)
        assert y.shape == want.shape, (k, f, p, h, w)
        assert bool(((y - want.detach()).abs() <= 1e-13 * a + 1e-300).all()), (k, f, p, h, w)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        want.backward(dy)
        dx, da, terms = R.downsample_bwd(dy, kern, h, w, f, p)
        assert bool(((dx - z.grad).abs() <= 1e-13 * da + 1e-300).all()), (k, f, p, h, w)
        assert 0 < terms <= k * k * (p + 1) ** 2 * y.shape[1] * y.shape[2]


# ----------------------------------------------------------------------------- the sweep's shapes and argument checks
def test_every_kernel_has_a_partial_last_block():
    for name, counts in R.kernel_threads().items():
        assert any(t > 256 and t % 256 for t in counts), name
    assert any(c[0] * c[1] * c[2] * c[3] > 256 and (c[0] * c[1] * c[2] * c[3]) % 256 for c in R.BOX_CASES)
    assert any(c[3] % 8 and c[7] and c[8] and c[9] and c[13] and c[14] and c[15] for c in R.BOX_CASES)


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + "._lib").lib()


def test_argument_checks_fail_before_any_launch(lib):
    """A box outside either tensor and an empty downsampler output return DSR_E_ARG (-1) -- also where the padded input is
    smaller than the kernel by less than the stride, so that a truncating division would call the output extent 1.  The
    pointers are never dereferenced: the calls return before a launch."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for idx, val in R.BOX_OUTSIDE:
        args = list(R.BOX_CASES[0])
        args[idx] = val
        assert lib.dsr_box_copy(p, p, *args, None) == -1, (idx, val)
        assert b"box" in lib.dsr_last_error()
    for k, f, pad, h, w in R.DS_EMPTY:
        assert lib.dsr_downsample_fwd(p, p, p, R.DS_NC, h, w, k, f, pad, None) == -1, (k, f, pad, h, w)
        assert lib.dsr_downsample_bwd(p, p, p, R.DS_NC, h, w, k, f, pad, None) == -1, (k, f, pad, h, w)
