"""GPU: float64 / exact-grid parity sweep of the resampling kernels of csrc/resample.hip through the raw C ABI, in bf16 and fp16
(reference and case tables: resample_ref.py; the reference against float64 torch, representability of the exact regime and the
table families: test_host_resample.py).

Exact regime: data on integer grids whose float64 results are representable in both storage types, so every output must EQUAL
the reference; copies (max-pool forward, nearest forward, box copy) run on arbitrary 16-bit patterns and are compared as int16.
Rounded regime: N(0,1) data against  |got - ref| <= u16 (|ref| + delta) + delta + floor,  delta = k 2^-24 A  (R.bound16), where
A is the sum of the absolute terms of the result and k the number of fp32 roundings on a term's way through the kernel, counted
from the kernel's arithmetic and stated at each check; fp32 outputs use delta alone (R.bound32).  No bound was read off a kernel.
Every output of a call sits inside a sentinel-filled buffer (canaries.py) whose margins must come back untouched."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

import resample_ref as R
from canaries import Canaries

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
E_ARG = -1


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def eq_nan(a, b):
    return (a == b) | (a.isnan() & b.isnan())


def same(got, want, what):
    """Numeric equality with the float64 reference (-0 equals +0; NaN equals NaN), with the first differing positions."""
    got, want = got.detach().cpu().to(torch.float64), want.to(torch.float64)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    bad = (~eq_nan(got, want)).nonzero()
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ; first at {bad[:6].tolist()}: got {got[i].item()} "
                             f"want {want[i].item()}")


def within(got, ref, bound, what):
    got, ref = got.detach().cpu().to(torch.float64), ref.to(torch.float64)
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        b = bound + torch.zeros_like(err)
        ratio = torch.where(bad, err / b.clamp_min(1e-300), torch.zeros_like(err))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} beyond the bound; first at {list(i)}: got {got[i].item()!r} "
                             f"ref {ref[i].item()!r} err {err[i].item():.3e} bound {b[i].item():.3e}; largest err / bound "
                             f"{float(ratio.max()):.3f}")


class Calls:
    """The entry points, each output inside a canary buffer.  Operands stay alive until the canaries are checked."""

    def __init__(self, dev, dtype=R.BF16):
        self.L = P("_lib")
        self.lib = self.L.lib()
        self.dev, self.dtype, self.tdt = dev, dtype, R.DTYPES[dtype]
        self.can = Canaries(dev)
        self.keep = []

    def up16(self, t):
        """float64 -> the 16-bit storage type on the device; the values must be representable."""
        out = t.to(torch.float32).to(self.tdt)
        assert bool(eq_nan(out.to(torch.float64), t.to(torch.float64)).all()), "operand not representable"
        return self.hold(out)

    def hold(self, t):
        """Host tensor -> device (an empty operand becomes a dummy vector: the entry points refuse NULL)."""
        t = t.contiguous().to(self.dev) if t.numel() else torch.zeros(8, dtype=t.dtype, device=self.dev)
        self.keep.append(t)
        return t

    def op(self, name, ins, out_shape, n, h, w, cp):
        """dsr_<name>(dtype, ins..., out, N, H, W, Cp, stream): the nine pool / upsampler entry points share this form."""
        out = self.can.alloc(out_shape, self.tdt, name)
        self.L.check(getattr(self.lib, "dsr_" + name)(self.dtype, *[ptr(t) for t in ins], ptr(out), n, h, w, cp, stream()))
        return out


# ----------------------------------------------------------------------------- exact regime
@pytest.mark.parametrize("dtype", DT)
def test_exact_pools_and_upsamplers(dev, dtype):
    """Every shape of the table (N 1 | 3; 1, 3, 5 channel groups; H, W from 2x2 to 16x18, odd ones included; 1x1, 1x5, 4x1 for
    the upsamplers and the average-pool adjoint), on the integer grids: max pool forward / backward / ReLU-masked backward,
    average pool and its adjoint, nearest forward and adjoint, bilinear forward and adjoint all EQUAL the float64 reference;
    the bilinear pair satisfies <fwd(x), dy> == <x, bwd(dy)> on the kernels' own outputs."""
    k = Calls(dev, dtype)
    todo, pairs = [], []
    for n, h, w, cp in R.shapes(thin=True):
        d = R.exact_case(n, h, w, cp)
        tag = f"{(n, h, w, cp)} "
        full, up, low = (n, h, w, cp), (n, 2 * h, 2 * w, cp), (n, h // 2, w // 2, cp)
        bx, bdy = k.up16(d["bil_x"]), k.up16(d["bil_dy"])
        by, bdx = k.op("bilinear2x_fwd", [bx], up, n, h, w, cp), k.op("bilinear2x_bwd", [bdy], full, n, h, w, cp)
        todo += [(by, d["bil_y"], tag + "bilinear fwd"), (bdx, d["bil_dx"], tag + "bilinear bwd")]
        pairs.append((by, d["bil_dy"], d["bil_x"], bdx, tag))
        todo.append((k.op("nearest2x_fwd", [bx], up, n, h, w, cp), R.nearest2x_fwd(d["bil_x"]), tag + "nearest fwd"))
        todo.append((k.op("nearest2x_bwd", [k.up16(d["near_dy"])], full, n, h, w, cp), d["near_dx"], tag + "nearest bwd"))
        todo.append((k.op("avgpool2_bwd", [k.up16(d["avg_dy"])], full, n, h, w, cp), d["avg_dx"], tag + "avgpool bwd"))
        if h < 2 or w < 2:
            continue
        todo.append((k.op("avgpool2_fwd", [k.up16(d["avg_x"])], low, n, h, w, cp), d["avg_y"], tag + "avgpool fwd"))
        mx, mdy, rx = k.up16(d["max_x"]), k.up16(d["max_dy"]), k.up16(d["relu_x"])
        todo.append((k.op("maxpool2_fwd", [mx], low, n, h, w, cp), R.maxpool2_fwd(d["max_x"]), tag + "maxpool fwd"))
        todo.append((k.op("maxpool2_bwd", [mx, mdy], full, n, h, w, cp), d["max_dx"], tag + "maxpool bwd"))
        todo.append((k.op("maxpool2_relu_bwd", [rx, mdy], full, n, h, w, cp), d["relu_dx"], tag + "maxpool relu bwd"))
    k.can.check()
    for got, want, what in todo:
        same(got, want, what)
    for by, dy, x, bdx, tag in pairs:
        assert float((by.cpu().double() * dy).sum()) == float((x * bdx.cpu().double()).sum()), tag + "bilinear adjoint identity"


@pytest.mark.parametrize("dtype", DT)
def test_copies_are_bit_exact(dev, dtype):
    """Arbitrary 16-bit patterns (NaNs with payloads, infinities, subnormals, signed zeros planted): nearest forward returns the
    very bits; max-pool forward returns the bits of the element the reference's scan ends on (where that element is a NaN, a
    NaN: the value passes through fp32 and its payload is not part of the contract)."""
    k = Calls(dev, dtype)
    todo = []
    for n, h, w, cp in R.shapes():
        bits = R.bits16(R._gen(2, n, h, w, cp, dtype), (n, h, w, cp), dtype)
        x = k.hold(bits.view(k.tdt))
        x64 = bits.view(k.tdt).to(torch.float64)
        _, arg = R.maxpool2_scan(x64)
        todo.append(("max", k.op("maxpool2_fwd", [x], (n, h // 2, w // 2, cp), n, h, w, cp), R.take_by_arg(bits, arg), (n, h, w, cp)))
        todo.append(("copy", k.op("nearest2x_fwd", [x], (n, 2 * h, 2 * w, cp), n, h, w, cp), R.nearest2x_fwd(bits), (n, h, w, cp)))
    k.can.check()
    for kind, got, want, shape in todo:
        gb = got.cpu().view(torch.int16)
        if kind == "copy":
            assert torch.equal(gb, want), f"nearest fwd {shape}"
        else:
            nan = want.view(k.tdt).isnan()
            assert bool((got.cpu().isnan() == nan).all()) and bool(((gb == want) | nan).all()), f"maxpool fwd {shape}"


@pytest.mark.parametrize("dtype", DT)
def test_maxpool_edge_windows(dev, dtype):
    """nn.MaxPool2d's rule at the edges: a NaN at each of the four positions and two or four together propagates, and the LAST
    NaN takes the gradient; +Inf wins, -Inf loses, an all -Inf window gives -Inf; all-equal windows and pairwise ties hand the
    gradient to the FIRST maximum; a dy of Inf or NaN reaches exactly one input; the trailing odd row and column (holding +Inf)
    are never read and get gradient 0.  Every channel lane of a vector holds a different window.  ReLU-masked form on ReLU
    outputs: an all-zero window gives gradient 0, a +Inf maximum passes its gradient."""
    k = Calls(dev, dtype)
    x, dy = R.edge_case(R.MAXPOOL_EDGES)
    n, h, w, cp = x.shape
    xd, dyd = k.up16(x), k.up16(dy)
    y = k.op("maxpool2_fwd", [xd], (n, 1, w // 2, cp), n, h, w, cp)
    dx = k.op("maxpool2_bwd", [xd, dyd], (n, h, w, cp), n, h, w, cp)
    rx, rdy = R.edge_case(R.RELU_EDGES)
    rn, rh, rw, _ = rx.shape
    rdx = k.op("maxpool2_relu_bwd", [k.up16(rx), k.up16(rdy)], (rn, rh, rw, cp), rn, rh, rw, cp)
    ry = k.op("maxpool2_fwd", [k.up16(rx)], (rn, 1, rw // 2, cp), rn, rh, rw, cp)
    k.can.check()
    same(y, R.maxpool2_fwd(x), "forward")
    assert int(y.isnan().sum()) == int(R.maxpool2_fwd(x).isnan().sum()) > 0
    same(dx, R.maxpool2_bwd(x, dy), "backward")
    dxc = dx.cpu().double()
    assert float(dxc[:, 2].abs().sum()) == 0.0 and float(dxc[:, :, -1].abs().sum()) == 0.0
    assert int(((dxc != 0) | dxc.isnan()).sum()) == int(((dy != 0) | dy.isnan()).sum())
    same(ry, R.maxpool2_fwd(rx), "forward on ReLU outputs")
    want = R.maxpool2_bwd(rx, rdy, relu_mask=True)
    same(rdx, want, "ReLU-masked backward")
    zero, inf = R.RELU_EDGES.index((0, 0, 0, 0)), R.RELU_EDGES.index((R.INF, 1, 2, 3))
    got = rdx.cpu().double()
    assert float(got[0, :2, 2 * zero:2 * zero + 2, 0].abs().sum()) == 0.0
    assert eq_nan(got[0, 0, 2 * inf, 0], rdy[0, 0, inf, 0]) and float(got[0, :2, 2 * inf:2 * inf + 2, 0].nan_to_num(1.0).abs().sum()) > 0


def test_fp16_finite_range(dev):
    """fp16, four times 65504: the average stays 65504 (an accumulation in 16 bits would overflow); the nearest adjoint's sum is
    +Inf, exactly as the reference rounds it."""
    k = Calls(dev, R.F16)
    x = torch.full((1, 2, 2, 8), R.F16_MAX, dtype=torch.float64)
    xd = k.up16(x)
    avg = k.op("avgpool2_fwd", [xd], (1, 1, 1, 8), 1, 2, 2, 8)
    near = k.op("nearest2x_bwd", [xd], (1, 1, 1, 8), 1, 1, 1, 8)
    k.can.check()
    same(avg, R.r16(R.avgpool2_fwd(x)[0], R.F16), "avgpool")
    assert float(avg.float().min()) == R.F16_MAX
    same(near, R.r16(R.nearest2x_bwd(x)[0], R.F16), "nearest adjoint")
    assert bool(near.isinf().all())


# ----------------------------------------------------------------------------- rounded regime
@pytest.mark.parametrize("dtype", DT)
def test_rounded_pools_and_upsamplers(dev, dtype):
    """N(0,1) data, every shape.  Roundings k of a term on its way to the fp32 result (then one rounding to 16 bits, the u16 term):
      average pool        (a + b + c + d) * 0.25: three additions, the product is exact                         k = 3
      average-pool adjoint  dy * 0.25 is exact in fp32                                                           k = 0
      nearest adjoint     (a + b) + (c + d): three additions                                                     k = 3
      bilinear forward    weights 0, 1/4, 3/4, 1: inner product, inner sum, outer product, outer sum             k = 4
      bilinear adjoint    at most 3 x 3 outputs reach an input: one product (wy * wx is exact) and <= 9 additions  k = 10
    Max pool forward and both backward forms select, so they stay equalities on real data."""
    k = Calls(dev, dtype)
    todo = []
    for n, h, w, cp in R.shapes(thin=True):
        g = R._gen(4, n, h, w, cp, dtype)
        tag = f"{(n, h, w, cp)} "
        full, up, low = (n, h, w, cp), (n, 2 * h, 2 * w, cp), (n, h // 2, w // 2, cp)
        x, dy_up, dy_low = R.real16(g, full, dtype), R.real16(g, up, dtype), R.real16(g, low, dtype)
        xd, dud = k.up16(x), k.up16(dy_up)
        ref, a = R.bilinear2x_fwd(x)
        todo.append((k.op("bilinear2x_fwd", [xd], up, n, h, w, cp), ref, R.bound16(ref, a, 4, dtype), tag + "bilinear fwd"))
        ref, a = R.bilinear2x_bwd(dy_up)
        todo.append((k.op("bilinear2x_bwd", [dud], full, n, h, w, cp), ref, R.bound16(ref, a, 10, dtype), tag + "bilinear bwd"))
        ref, a = R.nearest2x_bwd(dy_up)
        todo.append((k.op("nearest2x_bwd", [dud], full, n, h, w, cp), ref, R.bound16(ref, a, 3, dtype), tag + "nearest bwd"))
        ref = R.avgpool2_bwd(dy_low, h, w)
        todo.append((k.op("avgpool2_bwd", [k.up16(dy_low)], full, n, h, w, cp), ref, R.bound16(ref, ref.abs(), 0, dtype), tag + "avgpool bwd"))
        if h < 2 or w < 2:
            continue
        ref, a = R.avgpool2_fwd(x)
        todo.append((k.op("avgpool2_fwd", [xd], low, n, h, w, cp), ref, R.bound16(ref, a, 3, dtype), tag + "avgpool fwd"))
        dld = k.up16(dy_low)
        todo.append((k.op("maxpool2_fwd", [xd], low, n, h, w, cp), R.maxpool2_fwd(x), None, tag + "maxpool fwd"))
        todo.append((k.op("maxpool2_bwd", [xd, dld], full, n, h, w, cp), R.maxpool2_bwd(x, dy_low), None, tag + "maxpool bwd"))
        rx = x.clamp_min(0)
        todo.append((k.op("maxpool2_relu_bwd", [k.up16(rx), dld], full, n, h, w, cp), R.maxpool2_bwd(rx, dy_low, True), None,
                     tag + "maxpool relu bwd"))
    k.can.check()
    for got, ref, bound, what in todo:
        if bound is None:
            same(got, ref, what)
        else:
            within(got, ref, bound, what)


# ----------------------------------------------------------------------------- resize + crop + normalise
def _resize_tables(kind, dev):
    """(wy, wx) forward windows -> packed forward and transposed tables (host numpy), H, W, and the tuple of mean / std."""
    G = P("utils.GAN")
    if kind == "real":          # the product's own tables of a 9x downscale: windows wider than the register path holds
        tab = G.ResampleTables(144, 160, "cpu", resize_to=16, crop=12)
        wy, wx = tab.host
        h, w = 144, 160
    elif kind == "identity":    # as perceptual.py builds them: one weight of 1 per output
        h, w = 7, 9
        wy, wx = R.identity_windows(h), R.identity_windows(w)
    else:
        h, w = R.RESIZE_H, R.RESIZE_W
        wy, wx = R.resize_family()
    ty, tx = G._transpose_windows(wy, h), G._transpose_windows(wx, w)
    kt = max(max(len(v) for _, v in t) for t in (wy, wx, ty, tx))
    return [R.pack_tables(t, kt) for t in (wy, wx, ty, tx)], kt, h, w


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("kind", ["family", "identity", "real"])
def test_resize_norm(dev, kind, c, dtype):
    """dsr_resize_norm_fwd / _bwd on tables passed straight in, N = 2, C = 1 | 3, mean / std no powers of two.  `family`: hand-built
    windows with column counts 1, 15, 16, 17 and 40 in one launch (both sides of the kernel's nx <= 16 branch and its boundary;
    the wide windows sit at outputs > 0 and every table row differs), row counts 1 and 9; `identity`: perceptual.py's tables;
    `real`: ResampleTables(144, 160, resize_to=16, crop=12).  The backward reads utils.GAN._transpose_windows' tables.
    Forward: a term passes its product with wx, <= nx - 1 additions, the product with wy, <= ny - 1 additions, the subtraction
    of the mean, and the product with 1 / std (itself rounded): k = nx + ny + 3 with the launch's largest counts; A includes
    |mean| / std; output channels C..7 are exactly 0.  Backward (fp32 out): wy * wx, the product with dout, <= ny nx - 1
    additions, 1 / std and its product: k = ny nx + 3 with the transposed tables' largest counts."""
    k = Calls(dev, dtype)
    (ytab, xtab, tytab, txtab), kt, h, w = _resize_tables(kind, dev)
    oh, ow = len(ytab[0]), len(xtab[0])
    g = R._gen(6, c, dtype, len(kind))
    src = torch.randn(2, c, h, w, generator=g, dtype=torch.float32)
    dout = R.real16(g, (2, oh, ow, 8), dtype)                 # channels C..7 hold data too: the kernel must not let it in
    mean3, std3 = (C.c_float * 3)(*R.RESIZE_MEAN), (C.c_float * 3)(*R.RESIZE_STD)
    tabs = [[k.hold(torch.from_numpy(a)) for a in t] for t in (ytab, xtab, tytab, txtab)]
    out = k.can.alloc((2, oh, ow, 8), k.tdt, "resize_norm_fwd out")
    k.L.check(k.lib.dsr_resize_norm_fwd(dtype, ptr(k.hold(src)), ptr(out), 2, c, h, w, oh, ow, *[ptr(t) for t in tabs[0] + tabs[1]], kt,
                                        mean3, std3, stream()))
    dsrc = k.can.alloc((2, c, h, w), torch.float32, "resize_norm_bwd dsrc")
    k.L.check(k.lib.dsr_resize_norm_bwd(dtype, ptr(k.up16(dout)), ptr(dsrc), 2, c, h, w, oh, ow, *[ptr(t) for t in tabs[2] + tabs[3]], kt,
                                        std3, stream()))
    k.can.check()
    ref, a = R.resize_norm_fwd(src.double(), ytab, xtab, R.RESIZE_MEAN, R.RESIZE_STD)
    kf = int(xtab[1].max()) + int(ytab[1].max()) + 3
    within(out, ref, R.bound16(ref, a, kf, dtype), f"{kind} forward")
    assert float(out[..., c:].float().abs().sum()) == 0.0, "pad channels"
    ref, a = R.resize_norm_bwd(dout, tytab, txtab, R.RESIZE_STD, c, h, w)
    kb = int(tytab[1].max()) * int(txtab[1].max()) + 3
    within(dsrc, ref, R.bound32(a, kb), f"{kind} backward")
    if kind != "identity":          # the launch ran the generic loop; the family also the register path beside it
        assert int(xtab[1].max()) > 16 and (kind == "real" or int(xtab[1].min()) <= 16)


# ----------------------------------------------------------------------------- box copy
def test_box_copy(dev):
    """Arbitrary 16-bit patterns; nonzero source and destination offsets in y, x and channel; C no multiple of 8; a launch of 35
    blocks and a part of one.  The whole destination is compared as int16: the box holds the source's bits, everything else
    its sentinel.  A box outside either tensor returns DSR_E_ARG and leaves the destination untouched."""
    k = Calls(dev)
    todo = []
    for case in R.BOX_CASES:
        n, bh, bw, c, sh, sw, scp, sy0, sx0, cs0, dh, dw, dcp, dy0, dx0, cd0 = case
        bits = R.bits16(R._gen(8, *case), (n, sh, sw, scp), R.BF16)
        dst = k.can.alloc((n, dh, dw, dcp), torch.bfloat16, "box_copy dst")
        before = dst.cpu().view(torch.int16)
        k.L.check(k.lib.dsr_box_copy(ptr(k.hold(bits)), ptr(dst), *case, stream()))
        todo.append((dst, R.box_copy(bits, before, n, bh, bw, c, sy0, sx0, cs0, dy0, dx0, cd0), case))
    src = k.hold(R.bits16(R._gen(9), (2, 7, 9, 24), R.BF16))
    dst = k.can.alloc((2, 6, 8, 40), torch.bfloat16, "box_copy dst of the refused calls")
    for idx, val in R.BOX_OUTSIDE:
        args = list(R.BOX_CASES[0])
        args[idx] = val
        assert k.lib.dsr_box_copy(ptr(src), ptr(dst), *args, stream()) == E_ARG, (idx, val)
    k.can.check()
    assert k.can.untouched(dst)
    for got, want, case in todo:
        assert torch.equal(got.cpu().view(torch.int16), want), case


# ----------------------------------------------------------------------------- fixed-kernel downsampler
def test_downsampler(dev):
    """dsr_downsample_fwd / _bwd, fp32, a non-symmetric kernel, NC = 3: k 3 | 4 | 8, f 1 .. 4, p 0 | 1 | k // 2, H and W from
    1, 2, 5, 9, 13 wherever the output is non-empty -- sizes not divisible by f, H = 1 (both replicate ends fold onto one row),
    p >= H.  Forward: a term is one product and <= k^2 - 1 additions away from the result: k_r = k^2.  Adjoint: one product and
    <= T - 1 additions, T the largest number of terms any input element collects (counted by the reference): k_r = T."""
    k = Calls(dev)
    todo = []
    for kk, f, p, h, w in R.ds_cases():
        kern = R.ds_kernel(kk)
        g = R._gen(12, kk, f, p, h, w)
        x = torch.randn(R.DS_NC, h, w, generator=g, dtype=torch.float32)
        oh, ow = R.ds_out(h, kk, f, p), R.ds_out(w, kk, f, p)
        dy = torch.randn(R.DS_NC, oh, ow, generator=g, dtype=torch.float32)
        kd = k.hold(kern.float())
        y = k.can.alloc((R.DS_NC, oh, ow), torch.float32, "downsample_fwd y")
        dx = k.can.alloc((R.DS_NC, h, w), torch.float32, "downsample_bwd dx")
        k.L.check(k.lib.dsr_downsample_fwd(ptr(k.hold(x)), ptr(kd), ptr(y), R.DS_NC, h, w, kk, f, p, stream()))
        k.L.check(k.lib.dsr_downsample_bwd(ptr(k.hold(dy)), ptr(kd), ptr(dx), R.DS_NC, h, w, kk, f, p, stream()))
        todo.append((y, dx, x.double(), dy.double(), kern, (kk, f, p, h, w)))
    # an empty output is an error and launches nothing -- also where (H + 2p - k) / f + 1 truncates to 1
    y = k.can.alloc((R.DS_NC, 4, 4), torch.float32, "y of the refused calls")
    x = k.hold(torch.zeros(R.DS_NC, 13, 13))
    for kk, f, p, h, w in R.DS_EMPTY:
        kd = k.hold(R.ds_kernel(kk).float())
        assert k.lib.dsr_downsample_fwd(ptr(x), ptr(kd), ptr(y), R.DS_NC, h, w, kk, f, p, stream()) == E_ARG, (kk, f, p, h, w)
        assert k.lib.dsr_downsample_bwd(ptr(x), ptr(kd), ptr(y), R.DS_NC, h, w, kk, f, p, stream()) == E_ARG, (kk, f, p, h, w)
    k.can.check()
    assert k.can.untouched(y)
    for y, dx, x, dy, kern, case in todo:
        kk, f, p, h, w = case
        ref, a = R.downsample_fwd(x, kern, f, p)
        within(y, ref, R.bound32(a, kk * kk), f"forward {case}")
        ref, a, terms = R.downsample_bwd(dy, kern, h, w, f, p)
        within(dx, ref, R.bound32(a, terms), f"backward {case}")


# ----------------------------------------------------------------------------- the pool inside a DIP block
def test_dip_max_downsample_block_does_not_hide_an_overflow(dev):
    """fp16, models.DIP.utils.conv blocks run by run_fused: a 1x1 conv whose weight is scaled so that its output overflows fp16 at
    ONE pixel (+Inf in two channels), then conv(..., stride=2, downsample_mode='max'), whose weights of opposite sign turn that
    pixel into Inf - Inf = NaN in every channel while its three window neighbours stay finite.  (A conv of finite fp16 operands
    accumulates in fp32 and can only overflow to +-Inf, which any maximum keeps; the NaN that a pool can lose needs the next
    conv.)  nn.MaxPool2d hands the NaN on: the pooled map and the loss are non-finite and dsr_amp_check on the gradients sets
    found_inf, so a DynamicLossScaler skips the step.  A pool that keeps the finite neighbour instead reports a finite loss."""
    U, F = P("models.DIP.utils"), P("functional")
    L = P("_lib")
    F.clear_pack_cache()
    c, hw, big = 8, 8, (3, 5)
    seq = nn.Sequential()
    U.add(seq, U.conv(c, c, 1, bias=True, pad='zero'))
    U.add(seq, U.conv(c, c, 1, 2, bias=True, pad='zero', downsample_mode='max'))
    conv1, conv2 = seq[0][0], seq[1][0]
    assert isinstance(seq[1][1], nn.MaxPool2d)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        conv1.weight.copy_((torch.eye(c) * 60000.0).reshape(c, c, 1, 1))              # the scaled weight
        conv1.bias.zero_()
        w2 = (torch.randint(-4, 5, (c, c), generator=g).float() / 1024.0)
        w2[:, 0], w2[:, 1] = 1.0 / 1024.0, -1.0 / 1024.0
        conv2.weight.copy_(w2.reshape(c, c, 1, 1))
        conv2.bias.zero_()
    seq.to(dev).train()
    x = torch.full((1, c, hw, hw), 0.25)
    x[0, :, big[0], big[1]] = 0.5
    x[0, :2, big[0], big[1]] = 2.0                                                     # 2 * 60000 > 65504
    # the premise, in torch on the host with fp16 storage between the layers
    y1 = TF.conv2d(x.half().float(), conv1.weight.detach().cpu().half().float()).half()
    assert int(y1.isinf().sum()) == 2 and bool(y1[0, :2, big[0], big[1]].isinf().all()) and not bool(y1.isnan().any())
    y2 = TF.conv2d(y1.float(), conv2.weight.detach().cpu().half().float()).half()
    assert int(y2.isnan().sum()) == c and bool(y2[0, :, big[0], big[1]].isnan().all()) and bool(y2.nan_to_num(0.0).isfinite().all())
    want = TF.max_pool2d(y2.float(), 2, 2)
    assert int(want.isnan().sum()) == c
    out16, cout = U.run_fused(seq, F.ToNHWC.apply(x.to(dev), torch.float16), c, True)
    assert out16.dtype == torch.float16 and cout == c and tuple(out16.shape) == (1, hw // 2, hw // 2, c)
    out = F.ToNCHW.apply(out16, c)
    loss = F.mse_loss(out, torch.zeros_like(out))
    loss.backward()
    torch.cuda.synchronize()
    got = out.detach().cpu()
    assert bool((got.isnan() == want.isnan()).all()), "the pooled map lost (or invented) a NaN"
    assert torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))
    assert not bool(torch.isfinite(out16).all()) and not bool(torch.isfinite(loss))
    grads = [p.grad for p in seq.parameters()]
    assert all(gr is not None and gr.dtype == torch.float32 for gr in grads)
    found = torch.zeros(1, device=dev)
    n = len(grads)
    L.check(L.lib().dsr_amp_check(n, (C.c_void_p * n)(*[gr.data_ptr() for gr in grads]), (C.c_size_t * n)(*[gr.numel() for gr in grads]),
                                  ptr(found), stream()))
    assert found.item() == 1.0
