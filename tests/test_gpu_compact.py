"""GPU: SRVGGNetCompact on the HIP path (models/GAN/srvgg.py, csrc/conv_compact.hip, csrc/pw_compact.hip) against the float64
yardstick tests/compact_ref.py.

1. dsr_conv_prelu_c_fwd and dsr_conv_shuffle_add_fwd on exact-integer operands: compared with ==, every element outside the
   output untouched, also past the launcher's grid cap and with the optional operands NULL;
2. the same launches on float data: a derived per-element bound, and the same bits under every partition (max_blocks);
3. the pointwise kernels: exact on integers, the slope gradient's bound on float data, pixel counts taken from the query;
4. whole networks, fused and composed, against the float64 network with the storage-model network as the floor, with the
   launch counts of each form;
5. gradients of the composed form (tests/parity_util.compare_grads), slopes included, some of them negative;
6. the training recipe, HIP-graph replay, a captured fused forward after an optimiser step;
7. the inference surface (tiles, self-ensemble, evaluate_generator, checkpoints).

The head (3 -> 64 from 8 stored channels) runs as dsr_conv_fwd + one dsr_pw_prelu_c_fwd pass in the fused form too
(models/GAN/srvgg.py says why), so the fused form's count of pointwise PReLU passes is exactly one, not zero."""
import ctypes as C
import importlib
import os

import pytest
import torch

import compact_ref as R
import parity_util
from oracle import filler

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
MARGIN = 1024         # sentinel elements on each side of a raw buffer
SENTINEL = 7777.0


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


# ----------------------------------------------------------------------------- raw launches
class Raw:
    """Device tensors inside sentinel-filled allocations; check() asserts the margins came back untouched."""

    def __init__(self, dev):
        self.dev, self.flats = dev, []

    def alloc(self, shape, dtype, values=None):
        numel = 1
        for s in shape:
            numel *= s
        flat = torch.full((numel + 2 * MARGIN,), SENTINEL, dtype=dtype, device=self.dev)
        if values is not None:
            flat[MARGIN:MARGIN + numel] = values.reshape(-1).to(self.dev)
        self.flats.append(flat)
        return flat[MARGIN:MARGIN + numel].view(shape)

    def nhwc(self, nchw64, dtype, exact=True):
        t = nchw64.permute(0, 2, 3, 1).contiguous().to(R.DTYPES[dtype])
        if exact:
            assert torch.equal(t.double(), nchw64.permute(0, 2, 3, 1)), "operand not representable"
        return self.alloc(tuple(t.shape), t.dtype, t)

    def check(self):
        torch.cuda.synchronize()
        for flat in self.flats:
            assert bool((flat[:MARGIN] == SENTINEL).all()) and bool((flat[-MARGIN:] == SENTINEL).all()), "write outside a tensor"


def _packed(wt64, n, h, w, dtype, dev):
    F, L = P("functional"), P("_lib")
    weight = wt64.float().to(dev)
    cout, cin = weight.shape[:2]
    wf, _ = F.packed_weights(weight, L.ConvDesc(dtype, n, h, w, cin, cout, 3, 3, 1, 1, 0), R.DTYPES[dtype])
    return wf, weight


def _f32(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _body(dev, dtype, x, wt, bias, slope, max_blocks=0, exact=True, bits=False):
    """One dsr_conv_prelu_c_fwd launch through the raw ABI: y [N,64,H,W] float64 (or its int16 patterns) on the host."""
    L = P("_lib")
    n, _, h, w = x.shape
    raw = Raw(dev)
    xb = raw.nhwc(x, dtype, exact)
    before = xb.clone()
    yb = raw.alloc((n, h, w, 64), R.DTYPES[dtype])
    wf, keep = _packed(wt, n, h, w, dtype, dev)
    b, s = _f32(bias, dev), _f32(slope, dev)
    d = L.CompactConv(dtype, n, h, w, xb.data_ptr(), wf.data_ptr(), _ptr(b), _ptr(s), yb.data_ptr(), max_blocks)
    L.check(L.lib().dsr_conv_prelu_c_fwd(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    raw.check()
    assert torch.equal(xb.view(torch.int16), before.view(torch.int16))
    if bits:
        return yb.view(torch.int16).cpu()
    return yb.double().permute(0, 3, 1, 2).contiguous().cpu()


def _tail(dev, dtype, x, wt, bias, base, s, max_blocks=0, exact=True):
    """One dsr_conv_shuffle_add_fwd launch through the raw ABI: out [N,C,sH,sW] fp32 on the host, between sentinel margins."""
    L = P("_lib")
    n, _, h, w = x.shape
    c = wt.shape[0] // (s * s)
    raw = Raw(dev)
    xb = raw.nhwc(x, dtype, exact)
    ob = raw.alloc((n, c, s * h, s * w), torch.float32)
    bb = None if base is None else raw.alloc(tuple(base.shape), torch.float32, base.float())
    wf, keep = _packed(wt, n, h, w, dtype, dev)
    b = _f32(bias, dev)
    d = L.CompactTail(dtype, n, h, w, c, s, xb.data_ptr(), wf.data_ptr(), _ptr(b), _ptr(bb), ob.data_ptr(), max_blocks)
    L.check(L.lib().dsr_conv_shuffle_add_fwd(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    raw.check()
    return ob.cpu()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,h,w,mb", R.EXACT_SHAPES, ids=lambda v: str(v))
def test_body_exact(dev, dtype, n, h, w, mb):
    """Integers in [-3, 3], ternary weights, integer bias, slopes from {0, +-2^k} that differ per channel: nothing to round."""
    x, wt, bias, slope = R.exact_body(n, h, w)
    want = R.r16(R.conv_prelu(x, wt, bias, slope), dtype)
    got = _body(dev, dtype, x, wt, bias, slope, mb)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("has_bias,has_slope", [(False, True), (True, False), (False, False)])
def test_body_exact_null_operands(dev, dtype, has_bias, has_slope):
    x, wt, bias, slope = R.exact_body(2, 9, 65)
    bias, slope = (bias if has_bias else None), (slope if has_slope else None)
    want = R.r16(R.conv_prelu(x, wt, bias, slope), dtype)
    got = _body(dev, dtype, x, wt, bias, slope)
    assert torch.equal(got, want), float((got - want).abs().max())


_CAP = {}


@pytest.mark.parametrize("dtype", DT)
def test_body_exact_natural_cap(dev, dtype):
    """No max_blocks: 65 images x 2 x 2 ragged tiles = 260 work items on the cap of 256 blocks, so blocks 0..3 take a second
    item after the hand-over under their last K-block."""
    n, h, w = R.CAP_SHAPE
    assert R.tiles(n, h, w) == 260 > R.GRID_CAP
    if not _CAP:                                        # operands and the float64 value: once for both types, never modified
        ops = R.exact_body(n, h, w)
        _CAP["ops"], _CAP["y"] = ops, R.conv_prelu(*ops)
    want = R.r16(_CAP["y"], dtype)
    got = _body(dev, dtype, *_CAP["ops"])
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("n,h,w,mb", R.EXACT_SHAPES[:3], ids=lambda v: str(v))
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tail_exact(dev, dtype, s, n, h, w, mb, with_base):
    """C s^2 = 3, 12, 27, 48: the fp32 output, bit for bit, between sentinel margins (a store outside [N][C][sH][sW] shows)."""
    x, wt, bias, base = R.exact_tail(n, h, w, s)
    base = base if with_base else None
    want = R.conv_tail(x, wt, bias, base, s)
    got = _tail(dev, dtype, x, wt, bias, base, s, mb)
    assert got.dtype == torch.float32 and torch.equal(got.double(), want), float((got.double() - want).abs().max())


@pytest.mark.parametrize("dtype", DT)
def test_tail_exact_null_bias_and_four_planes(dev, dtype):
    x, wt, bias, base = R.exact_tail(2, 9, 65, 4, c=4)                # C s^2 = 64: every row of the MFMA tile is a real output
    got = _tail(dev, dtype, x, wt, None, base, 4)
    assert torch.equal(got.double(), R.conv_tail(x, wt, None, base, 4))


@pytest.mark.parametrize("dtype", DT)
def test_body_float_bound_and_partitions(dev, dtype):
    """N(0, 1) data, N(0, 0.05) weights, slopes in [-1.5, 1.5].  Per element, none excluded:
        |y - y64| <= u |y64| + (9 * 64 + 4) 2^-24 A max(1, |slope_c|),  A = sum |x| |w| + |b|,
    and the same bits under max_blocks 0, 1, 3 (8 tiles: 8 blocks of one, one block of 8, three blocks of 3, 3 and 2)."""
    x, wt, bias, slope = R.float_body(dtype)
    y64 = R.conv_prelu(x, wt, bias, slope)
    bound = R.body_bound(y64, x, wt, bias, slope, dtype)
    got = _body(dev, dtype, x, wt, bias, slope, 0, exact=False)
    ratio = float(((got - y64).abs() / bound).max())
    print(f"body float {dtype}: max err {float((got - y64).abs().max()):.3e}, worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    runs = {mb: _body(dev, dtype, x, wt, bias, slope, mb, exact=False, bits=True) for mb in R.FLOAT_PARTITIONS}
    for mb in R.FLOAT_PARTITIONS[1:]:
        assert torch.equal(runs[mb], runs[0]), mb


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tail_float_bound_and_partitions(dev, dtype, s):
    """|out - out64| <= (9 * 64 + 3) 2^-24 (A + |base|): fp32 throughout, no 16-bit term; same bits under max_blocks 0, 1, 3."""
    x, wt, bias, base = R.float_tail(dtype, s)
    out64 = R.conv_tail(x, wt, bias, base, s)
    bound = R.tail_bound(x, wt, bias, base, s)
    runs = {mb: _tail(dev, dtype, x, wt, bias, base, s, mb, exact=False) for mb in R.FLOAT_PARTITIONS}
    ratio = float(((runs[0].double() - out64).abs() / bound).max())
    print(f"tail float {dtype} s={s}: max err {float((runs[0].double() - out64).abs().max()):.3e}, worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    for mb in R.FLOAT_PARTITIONS[1:]:
        assert torch.equal(runs[mb].view(torch.int32), runs[0].view(torch.int32)), mb


# ----------------------------------------------------------------------------- pointwise kernels
def _pixel_counts(lib):
    """Pixel counts from the partial-row query: one row, a ragged last row, one row more than the fold's width."""
    ppr = next(p for p in range(1, 1 << 16) if lib.dsr_pw_prelu_c_rows(p + 1) == 2)       # pixels of a full row
    fold = lib.dsr_pw_prelu_c_fold_width()
    counts = [ppr, 3 * ppr + 7, fold * ppr + 1]
    assert [lib.dsr_pw_prelu_c_rows(p) for p in counts] == [1, 4, fold + 1]
    return counts


def _nchw(t, c):
    return t[..., :c].double().permute(0, 3, 1, 2).contiguous().cpu()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c", [64, 12])
def test_pointwise_prelu_exact(dev, dtype, c):
    """Integers in [-6, 6] (zeros among them), slopes from {0, +-2^k}: forward, dz and the slope gradient compared with ==.
    dz at z == 0 is dy * slope and the slope gradient's term there is 0: torch's rules.  c = 12: 16 stored channels, the pad
    channels come back zero."""
    F = P("functional")
    lib = P("_lib").lib()
    cp = (c + 7) // 8 * 8
    slope = R.exact_slopes(c)
    for p in _pixel_counts(lib):
        g = torch.Generator().manual_seed(p + c)
        z = R.small_ints(g, (1, c, 1, p), 6)
        dy = R.small_ints(g, (1, c, 1, p), 3)
        pad = lambda t: torch.cat([t, torch.zeros(1, cp - c, 1, p, dtype=torch.float64)], 1).permute(0, 2, 3, 1).contiguous()
        zd = pad(z).to(R.DTYPES[dtype]).to(dev).requires_grad_(True)
        sd = slope.float().to(dev).requires_grad_(True)
        y = F.PReLUChannel.apply(zd, sd)
        assert torch.equal(_nchw(y.detach(), c), R.prelu_c(z, slope))
        assert not bool(y.detach()[..., c:].any())
        y.backward(pad(dy).to(R.DTYPES[dtype]).to(dev))
        dz, dslope = R.prelu_bwd(dy, z, slope)
        assert torch.equal(_nchw(zd.grad, c), dz), p
        assert torch.equal(sd.grad.double().cpu(), dslope), (p, float((sd.grad.double().cpu() - dslope).abs().max()))
        assert bool((z == 0).any())


@pytest.mark.parametrize("dtype", DT)
def test_pointwise_prelu_float_bound_and_equal_bits(dev, dtype):
    """dslope within P 2^-24 sum |dy z| of the float64 sum; dz the product rounded to 16 bits; two runs give equal bits."""
    F = P("functional")
    lib = P("_lib").lib()
    p = _pixel_counts(lib)[2]
    g = torch.Generator().manual_seed(3)
    t16 = lambda t: t.to(R.DTYPES[dtype])
    z = t16(torch.randn(1, 64, 1, p, generator=g, dtype=torch.float64))
    dy = t16(torch.randn(1, 64, 1, p, generator=g, dtype=torch.float64))
    slope = (torch.rand(64, generator=g, dtype=torch.float64) * 3.0 - 1.5).float()
    slope[5] = 0.0
    runs = []
    for _ in range(2):
        zd = z.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        sd = slope.to(dev).requires_grad_(True)
        F.PReLUChannel.apply(zd, sd).backward(dy.permute(0, 2, 3, 1).contiguous().to(dev))
        runs.append((zd.grad.clone(), sd.grad.clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(runs[0][1], runs[1][1])
    dz, dslope = R.prelu_bwd(dy, z, slope)
    # dz is the product dy * slope (exact in float64) rounded to 16 bits, either directly (a mixed-precision multiply that
    # rounds once) or through fp32 as the storage model does: never farther from the product than the storage model's value
    got_dz = _nchw(runs[0][0], 64)
    assert bool(((got_dz - dz).abs() <= (R._store(dz, dtype) - dz).abs()).all())
    bound = p * 2.0 ** -24 * (dy.double() * z.double()).abs().sum(dim=(0, 2, 3))
    ratio = float(((runs[0][1].double().cpu() - dslope).abs() / bound).max())
    print(f"dslope float {dtype} P={p}: worst err / bound {ratio:.5f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_shuffle_add_exact(dev, s):
    F = P("functional")
    g = torch.Generator().manual_seed(s)
    t, base = R.small_ints(g, (2, 3 * s * s, 5, 7), 50), R.small_ints(g, (2, 3, 5, 7), 50)
    dout = R.small_ints(g, (2, 3, 5 * s, 7 * s), 50)
    dt64, dbase64 = R.shuffle_add_bwd(dout, s)
    for want_base_grad in (True, False):
        td = t.float().to(dev).requires_grad_(True)
        bd = base.float().to(dev).requires_grad_(want_base_grad)
        out = F.ShuffleAdd.apply(td, bd, s)
        assert torch.equal(out.detach().double().cpu(), R.shuffle_add(t, base, s))
        out.backward(dout.float().to(dev))
        assert torch.equal(td.grad.double().cpu(), dt64)
        assert (bd.grad is None) == (not want_base_grad)
        if want_base_grad:
            assert torch.equal(bd.grad.double().cpu(), dbase64)


# ----------------------------------------------------------------------------- networks
def _net(dev, dtype=torch.bfloat16, salt=0, **kw):
    """A module on closed-form weights; PReLU slopes redrawn in [-0.5, 0.5], so that some are negative."""
    net = P("models.GAN.srvgg").SRVGGNetCompact(**kw)
    sd = filler.fill_state_dict(net.state_dict(), salt=salt)
    for k, v in sd.items():
        if v.dim() == 1 and k.endswith(".weight"):
            sd[k] = filler.tensor("slope:" + k, tuple(v.shape), 0.5, 0.0, salt=salt)
    net.load_state_dict(sd)
    net.to(dev)
    net.compute_dtype = dtype
    return net, sd


def _count(fn):
    """Run fn with the launch log on; returns (result, {entry point: launches})."""
    L = P("_lib")
    L.LAUNCH_LOG = log = []
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.LAUNCH_LOG = None
    counts = {}
    for name, _, _ in log:
        counts[name] = counts.get(name, 0) + 1
    return out, counts


NETS = [pytest.param(dict(num_conv=2, upscale=4), (1, 3, 12, 20), id="c2x4-12x20"),
        pytest.param(dict(num_conv=2, upscale=4), (2, 3, 9, 65), id="c2x4-9x65"),
        pytest.param(dict(num_conv=3, upscale=2), (1, 3, 16, 24), id="c3x2-16x24"),
        pytest.param(dict(num_conv=2, upscale=3), (1, 3, 12, 20), id="c2x3-12x20"),
        pytest.param(dict(num_conv=2, upscale=4, num_feat=32), (1, 3, 12, 20), id="f32-composed-only"),
        pytest.param(dict(num_conv=2, upscale=4, act_type="relu"), (1, 3, 12, 20), id="relu"),
        pytest.param(dict(num_conv=2, upscale=4, act_type="leakyrelu"), (1, 3, 12, 20), id="leakyrelu")]


@pytest.mark.parametrize("kw,shape", NETS)
def test_network_forward(dev, monkeypatch, kw, shape):
    """max|y_hip - y_f64| <= 2 E_floor + 1e-3 max|y_f64|, E_floor = max|y_sim - y_f64| (the storage-model yardstick of each
    form), for the fused no-grad forward, the composed forward, and their mutual difference (the larger floor).  Launches: the
    fused form is num_conv launches of dsr_conv_prelu_c_fwd and one of dsr_conv_shuffle_add_fwd, one pointwise PReLU pass (the
    head's) and no shuffle pass; the composed form issues none of the two; DSR_COMPACT_FUSED=0 gives the composed bits.

    Measured on the MI355X (bf16), E_floor fused / composed, errors fused / composed / mutual, max|y_f64|:
        num_conv=2 x4, 1x3x12x20   3.74e-3 / 3.71e-3,  3.74e-3 / 3.71e-3 / 1.60e-3,  1.52
        num_conv=2 x4, 2x3x9x65    4.81e-3 / 5.17e-3,  4.81e-3 / 5.17e-3 / 1.71e-3,  1.66
        num_conv=3 x2, 1x3x16x24   3.10e-3 / 3.07e-3,  3.10e-3 / 3.07e-3 / 1.91e-3,  1.62
        upscale=3,     1x3x12x20   3.74e-3 / 3.71e-3,  3.74e-3 / 3.71e-3 / 1.60e-3,  1.56
        num_feat=32,   1x3x12x20   3.75e-3 / 4.06e-3,  4.06e-3 / 4.06e-3 / 0 (one path),  1.56
        relu,          1x3x12x20   3.77e-3 / 3.77e-3,  3.77e-3 / 3.77e-3 / 2.4e-7,  1.47
        leakyrelu,     1x3x12x20   3.80e-3 / 3.70e-3,  3.80e-3 / 3.70e-3 / 8.8e-4,  1.53"""
    net, sd = _net(dev, **kw)
    assert any(float(v.min()) < 0 for k, v in sd.items() if v.dim() == 1 and k.endswith(".weight")) or kw.get("act_type")
    x = filler.tensor("in:compact" + str(shape), shape, 0.5, 0.5)
    s, nc = kw["upscale"], kw["num_conv"]
    act = kw.get("act_type")
    y64 = R.network(sd, x, s, act=act)
    floor_f = float((R.network(sd, x, s, dtype=R.BF16, act=act) - y64).abs().max())
    floor_c = float((R.network(sd, x, s, dtype=R.BF16, fused=False, act=act) - y64).abs().max())
    ymax = float(y64.abs().max())
    bound_f, bound_c = 2.0 * floor_f + 1e-3 * ymax, 2.0 * floor_c + 1e-3 * ymax
    xd = x.to(dev)
    with torch.no_grad():
        fused, counts = _count(lambda: net(xd))
    composed, ccounts = _count(lambda: net(xd))                      # grad mode on, parameters require grad
    monkeypatch.setenv("DSR_COMPACT_FUSED", "0")
    with torch.no_grad():
        off, ocounts = _count(lambda: net(xd))
    monkeypatch.delenv("DSR_COMPACT_FUSED")
    a, b = "dsr_conv_prelu_c_fwd", "dsr_conv_shuffle_add_fwd"
    if kw.get("num_feat", 64) == 64:
        assert counts.get(a, 0) == nc and counts.get(b, 0) == 1, counts
        assert counts.get("dsr_pw_prelu_c_fwd", 0) == 1 and counts.get("dsr_shuffle_add_f32", 0) == 0, counts
        assert counts.get("dsr_conv_fwd", 0) == 1, counts
    else:
        assert counts.get(a, 0) == 0 and counts.get(b, 0) == 0, counts
    for c in (ccounts, ocounts):
        assert c.get(a, 0) == 0 and c.get(b, 0) == 0, c
        assert c.get("dsr_pw_prelu_c_fwd", 0) == nc + 1 and c.get("dsr_shuffle_add_f32", 0) == 1 and c.get("dsr_conv_fwd", 0) == nc + 2, c
    assert torch.equal(off, composed.detach())
    e_f = float((fused.double().cpu() - y64).abs().max())
    e_c = float((composed.detach().double().cpu() - y64).abs().max())
    e_m = float((fused - composed.detach()).abs().max())
    print(f"network {kw} {shape}: E_floor fused {floor_f:.3e} composed {floor_c:.3e} bound {bound_f:.3e} / {bound_c:.3e} "
          f"fused {e_f:.3e} composed {e_c:.3e} mutual {e_m:.3e} max|y| {ymax:.3e}")
    assert tuple(fused.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and fused.dtype == torch.float32
    assert e_f <= bound_f and e_c <= bound_c and e_m <= max(bound_f, bound_c), (e_f, e_c, e_m, bound_f, bound_c)


def test_composed_gradients(dev):
    """Every parameter gradient (slopes included, some of them negative) and the input gradient of the composed form against
    the float64 network's, with the storage-model network (composed rounding points) as the floor: parity_util.compare_grads
    as it stands.  No gradient is NaN."""
    shape = (2, 3, 12, 20)
    net, sd = _net(dev, num_conv=2)
    assert sum(int((v < 0).sum()) for k, v in sd.items() if v.dim() == 1 and k.endswith(".weight")) > 10
    x = filler.tensor("in:compact_grad", shape, 0.5, 0.5)
    probe = filler.tensor("in:compact_probe", (2, 3, 48, 80))

    def ref_grads(dtype):
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        xi = x.double().clone().requires_grad_(True)
        y = R.network(leaves, xi, 4, dtype=dtype, fused=False)
        (y * probe.double()).sum().backward()
        out = {k: v.grad for k, v in leaves.items()}
        out["input"] = xi.grad
        return out

    ref, sim = ref_grads(None), ref_grads(R.BF16)
    xd = x.to(dev).requires_grad_(True)
    y, counts = _count(lambda: net(xd))
    assert counts.get("dsr_conv_prelu_c_fwd", 0) == 0 and counts.get("dsr_conv_shuffle_add_fwd", 0) == 0
    (y * probe.to(dev)).sum().backward()
    hip = {k: p.grad for k, p in net.named_parameters()}
    hip["input"] = xd.grad
    assert all(g is not None for g in hip.values())
    assert not any(bool(torch.isnan(g).any()) for g in hip.values())
    bad, table = parity_util.compare_grads(hip, ref, sim)
    worst = sorted(table.items(), key=lambda kv: kv[1][0])[:5]
    print("composed gradients, lowest cosines (cos_hip, cos_floor, ratio_hip, ratio_floor, numel):", worst)
    assert len(table) == len(ref) and not bad, bad


def _batch(dev):
    lr = filler.tensor("in:compact_lr", (16, 3, 8, 8), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:compact_hr", (16, 3, 32, 32), 0.5, 0.5).to(dev)
    return lr, hr


def _params(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_l1_step_lowers_the_loss_and_replays_from_a_graph(dev):
    O, S = P("optim"), P("steps")
    lr, hr = _batch(dev)

    def setup():
        net, _ = _net(dev, num_conv=2)
        net.train()
        opt = O.FusedAdam(net.parameters(), lr=1e-3)
        ema = O.WeightEMA(net, decay=0.9)
        return net, opt, ema

    net, opt, ema = setup()
    losses = []
    for _ in range(5):
        loss, fake = S.gen_l1_step(net, opt, lr, hr, ema=ema)
        losses.append(loss.clone())
    losses = [float(v) for v in losses]
    print("L1 over 5 steps:", losses)
    assert losses[-1] < losses[0] and all(v == v for v in losses)
    assert int(ema.n_averaged.item()) == 5

    # the same five steps, two eager and three replayed from a HIP graph: bit for bit
    net2, opt2, ema2 = setup()
    out = []
    graphed = S.GraphedStep(lambda: S.gen_l1_step(net2, opt2, lr, hr, ema=ema2), warmup=2)
    for _ in range(3):
        loss2, fake2 = graphed()
        out.append(loss2.clone())
    torch.cuda.synchronize()
    assert float(out[-1]) == losses[-1]
    assert torch.equal(fake2, fake)
    a, b = _params(net), _params(net2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["body.1.weight"], _net(dev, num_conv=2)[1]["body.1.weight"].to(dev))     # the slopes trained


def test_captured_fused_forward_sees_the_updated_weights_and_slopes(dev):
    O, S, M = P("optim"), P("steps"), P("models.GAN.srvgg")
    net, _ = _net(dev, num_conv=2)
    x = filler.tensor("in:compact_cap", (1, 3, 12, 20), 0.5, 0.5).to(dev)
    with torch.no_grad():
        eager = net(x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = net(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)
    # an optimiser step rewrites weights and slopes through raw pointers and refreshes the packed images in place: the replay
    # reads the slopes from the parameters' own storage and the images from theirs
    lr, hr = _batch(dev)
    opt = O.FusedAdam(net.parameters(), lr=1e-3)
    S.gen_l1_step(net, opt, lr, hr)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        after, counts = _count(lambda: net(x))
    assert counts.get("dsr_conv_prelu_c_fwd", 0) == 2 and counts.get("dsr_conv_shuffle_add_fwd", 0) == 1
    assert not torch.equal(after, eager)
    assert torch.equal(static, after)
    fresh = M.SRVGGNetCompact(num_conv=2)
    fresh.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    fresh.to(dev)
    with torch.no_grad():
        assert torch.equal(fresh(x), after)


# ----------------------------------------------------------------------------- inference surface
def test_super_resolve_tiles_ensemble_evaluate_and_checkpoints(dev, tmp_path):
    I, E, M = P("infer"), P("evaluate"), P("models.GAN.srvgg")
    net, _ = _net(dev, num_conv=2)
    lr = filler.tensor("in:compact_sr", (1, 3, 24, 40), 0.5, 0.5).to(dev)
    whole = I.super_resolve(net, lr)
    assert tuple(whole.shape) == (1, 3, 96, 160) and net.compute_dtype == torch.bfloat16
    assert net.receptive_halo() == 4
    tiled = I.super_resolve(net, lr, tile=8, halo=net.receptive_halo())
    assert torch.equal(tiled, whole)
    ens = I.super_resolve(net, lr, self_ensemble=True)
    singles = [I.d4_inverse(I.super_resolve(net, I.d4(lr, k)), k) for k in range(8)]
    mean = torch.stack(singles).double().mean(0).float()
    assert float((ens - mean).abs().max()) <= 1e-6
    pairs = [(filler.tensor(f"in:compact_ev{i}", (1, 3, 12, 16), 0.5, 0.5).to(dev),
              filler.tensor(f"in:compact_evhr{i}", (1, 3, 48, 64), 0.5, 0.5).to(dev), f"img{i}") for i in range(2)]
    res = E.evaluate_generator(net, pairs, with_ssim=False, y_channel=True)
    for key in ("psnr", "psnr_y"):
        assert len(res[key]) == 2 and all(v == v and abs(v) != float("inf") for v in res[key].values()), res
    # checkpoints: save / load into a fresh module, and BasicSR's {'params': ...} wrapping
    path = E.save_model(net, "compact", str(tmp_path))
    fresh = M.SRVGGNetCompact(**E.inspect_srvgg(torch.load(path, map_location="cpu", weights_only=True)))
    E.load_model(fresh, path).to(dev)
    assert torch.equal(I.super_resolve(fresh, lr), whole)
    wrapped = os.path.join(str(tmp_path), "wrapped.pth")
    torch.save({"params": {k: v.detach().cpu() for k, v in net.state_dict().items()}}, wrapped)
    fresh2 = E.load_model(M.SRVGGNetCompact(num_conv=2), wrapped).to(dev)
    assert torch.equal(I.super_resolve(fresh2, lr), whole)
