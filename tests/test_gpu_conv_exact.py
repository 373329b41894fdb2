"""GPU: exact-integer parity sweep of every convolution kernel, in bf16 and fp16 (reference and case table: conv_exact_ref.py).

Small-integer operands make every product and partial sum exact in fp32, so the result is independent of summation order, MFMA
shape and split-K; the only rounding left is the final store to 16 bits.  A kernel is right bit for bit or it is wrong: there is
no tolerance anywhere in this file.  Regime A keeps every stored value representable (no rounding at all) and covers forward
with its epilogues, input gradient in its fused forms, weight gradient, bias / PReLU gradients and BatchNorm statistics; regime B
scales the operands up so that the outputs are rounded, a few hundred of them exact ties (expected: round to nearest even of the
exact value).  Every output and workspace of a raw C-ABI call sits in the middle of a larger sentinel-filled buffer whose
margins must come back untouched: an out-of-bounds store of a ragged tile shows up without any fault.  tests/
test_host_conv_exact.py proves, without a GPU, that the cases stay in their regimes and reach every kernel the dispatcher names."""
import ctypes as C
import importlib

import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
SENTINEL = 7777.0
MARGIN = 512          # elements on each side of an output


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


def nhwc(t, dtype, dev, cp=None):
    """float64 NCHW -> 16-bit NHWC on the device, real channels only: pad channels zero, as the product guarantees."""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cp or R.r8(c), dtype=R.DTYPES[dtype])
    out[..., :c] = t.permute(0, 2, 3, 1).to(R.DTYPES[dtype])
    assert torch.equal(out[..., :c].double(), t.permute(0, 2, 3, 1))
    return out.to(dev)


def nchw64(y, c):
    return y[..., :c].double().permute(0, 3, 1, 2).contiguous().cpu()


class Canaries:
    """Outputs allocated inside sentinel-filled buffers; check() asserts that nothing outside an output was written."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def alloc(self, shape, dtype, what):
        numel = 1
        for s in shape:
            numel *= int(s)
        flat = torch.full((numel + 2 * MARGIN,), SENTINEL, dtype=dtype, device=self.dev) if dtype != torch.uint8 else \
            torch.full((numel + 2 * MARGIN,), 0xA5, dtype=dtype, device=self.dev)
        self.bufs.append((flat, numel, what))
        return flat[MARGIN:MARGIN + numel].view(*shape) if numel else flat[MARGIN:MARGIN]

    def check(self):
        torch.cuda.synchronize()
        for flat, numel, what in self.bufs:
            lo, hi = flat[:MARGIN], flat[MARGIN + numel:]
            assert bool((lo == lo[0]).all()) and bool((hi == lo[0]).all()) and bool(lo[0] == flat.new_tensor(
                0xA5 if flat.dtype == torch.uint8 else SENTINEL)), f"store outside {what}"


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(t, dev):
    return None if t is None else t.to(torch.float32).contiguous().to(dev)


def desc_of(L, c, dtype):
    return L.ConvDesc(dtype, c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"], c["k"], c["stride"], c["pad"], c["mode"])


def pack(L, lib, d, w, dtype, dev):
    wf = torch.empty(lib.dsr_conv_packed_elems(C.byref(d), 0), dtype=R.DTYPES[dtype], device=dev)
    wd = torch.empty(lib.dsr_conv_packed_elems(C.byref(d), 1), dtype=R.DTYPES[dtype], device=dev)
    wdev = f32(w, dev)
    L.check(lib.dsr_conv_pack_weight(C.byref(d), ptr(wdev), ptr(wf), ptr(wd), stream()))
    return wf, wd


def same(got, want, what):
    """Numeric equality (-0 equals +0), with the first differing positions in the message."""
    got, want = got.double().cpu(), want.double()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ; first at {bad[:6].tolist()}: got "
                             f"{got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")


def raw_forward(L, lib, dev, c, dtype, r, wf, can, plain=False):
    """dsr_conv_fwd into canary buffers.  plain: no bias, activation or epilogue extras (regime B).  Returns (y, stats)."""
    d = desc_of(L, c, dtype)
    oh, ow = R.out_size(c["h"], c["w"], c["k"], c["stride"], c["pad"])
    cout, tdt = c["cout"], R.DTYPES[dtype]
    x = nhwc(r["x"], dtype, dev)
    ps, nchw, stats_on = (c["ps"], c["nchw"], c["stats"]) if not plain else (False, False, False)
    keep = [x]
    y = out32 = stats = None
    if nchw:
        out32 = can.alloc((c["n"], cout, oh, ow), torch.float32, "out_nchw_f32")
    elif ps:
        y = can.alloc((c["n"], 2 * oh, 2 * ow, R.r8(cout // 4)), tdt, "y (pixel shuffle)")
    else:
        y = can.alloc((c["n"], oh, ow, R.r8(cout)), tdt, "y")
    if stats_on:
        rows = lib.dsr_conv_stats_rows(C.byref(d))
        assert rows > 0
        stats = can.alloc((rows, 2, R.r8(cout)), torch.float32, "stats_partial")
    if plain:
        ep = L.Epilogue(R.ACT_NONE, 0.0, None, None, None, 0, None)
    else:
        prelu = torch.full((1,), c["slope"], device=dev) if c["act"] == R.ACT_PRELU else None
        bias = f32(r["b"], dev)
        sc = sh = res = None
        if c["fold"]:
            sc, sh = torch.zeros(R.r8(cout), device=dev), torch.zeros(R.r8(cout), device=dev)
            sc[:cout], sh[:cout] = f32(r["bn_scale"], dev), f32(r["bn_shift"], dev)
        if c["residual"]:
            res = nhwc(r["residual"], dtype, dev)
        keep += [prelu, bias, sc, sh, res]
        ep = L.Epilogue(c["act"], c["slope"], ptr(prelu), ptr(bias), ptr(stats), int(ps), ptr(out32), ptr(sc), ptr(sh), ptr(res))
    L.check(lib.dsr_conv_fwd(C.byref(d), ptr(x), ptr(wf), C.byref(ep), ptr(y), stream()))
    torch.cuda.synchronize()
    return (out32 if nchw else y), stats


def raw_dgrad(L, lib, dev, c, dtype, r, g, wd, can, variant):
    d = desc_of(L, c, dtype)
    gd = nhwc(g, dtype, dev)
    dx = can.alloc((c["n"], c["h"], c["w"], R.r8(c["cin"])), R.DTYPES[dtype], "dx")
    if variant == "add":
        assert lib.dsr_conv_dgrad_add_supported(C.byref(d)) == 1
        add = nhwc(r["addend"], dtype, dev)
        L.check(lib.dsr_conv_dgrad_add(C.byref(d), ptr(gd), ptr(wd), ptr(add), ptr(dx), stream()))
    elif variant in ("relu", "leaky"):
        assert lib.dsr_conv_dgrad_masked_supported(C.byref(d)) == 1
        xa = nhwc(r["x"], dtype, dev)
        L.check(lib.dsr_conv_dgrad_masked(C.byref(d), ptr(gd), ptr(wd), ptr(xa), r["mask_act"], 0.25, ptr(dx), stream()))
    else:
        wsz = lib.dsr_conv_dgrad_workspace(C.byref(d))
        ws = can.alloc((max(wsz, 16),), torch.uint8, "dgrad workspace")
        L.check(lib.dsr_conv_dgrad(C.byref(d), ptr(gd), ptr(wd), ptr(dx), ptr(ws), wsz, stream()))
    torch.cuda.synchronize()
    return dx


def raw_wgrad(L, lib, dev, c, dtype, r, can):
    d = desc_of(L, c, dtype)
    x, gd = nhwc(r["x"], dtype, dev), nhwc(r["g"], dtype, dev)
    dw = can.alloc((c["cout"], c["cin"], c["k"], c["k"]), torch.float32, "dw")
    wsz = lib.dsr_conv_wgrad_workspace(C.byref(d))
    assert wsz > 0
    ws = can.alloc((wsz,), torch.uint8, "wgrad workspace")
    L.check(lib.dsr_conv_wgrad(C.byref(d), ptr(x), ptr(gd), ptr(dw), ptr(ws), wsz, stream()))
    torch.cuda.synchronize()
    return dw


def set_env(monkeypatch, c):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_regime_a_raw_abi(dev, name, dtype, monkeypatch):
    """No rounding anywhere: y (NHWC, pixel-shuffled or fp32 NCHW), the BatchNorm statistics rows summed per channel, dx in
    the case's form (plain / + addend / masked) and dw equal the reference; pad channels are zero; canary margins intact."""
    L = P("_lib")
    lib = L.lib()
    r = R.layer_a(name)
    c = r["case"]
    set_env(monkeypatch, c)
    got = R.kernel_names(lib, c, dtype)
    assert all(w is None or w == g for w, g in zip(c["names"], got)), (got, c["names"])
    d = desc_of(L, c, dtype)
    wf, wd = pack(L, lib, d, r["w"], dtype, dev)
    can = Canaries(dev)
    y, stats = raw_forward(L, lib, dev, c, dtype, r, wf, can)
    dx = raw_dgrad(L, lib, dev, c, dtype, r, r["g"], wd, can, c["dgrad"]) if c["dgrad"] is not None else None
    dw = raw_wgrad(L, lib, dev, c, dtype, r, can) if c["names"][2] is not None else None
    can.check()
    cout = c["cout"]
    if c["nchw"]:
        same(y, r["y"], "out_nchw_f32")
    elif c["ps"]:
        same(nchw64(y, cout // 4), R.pixel_shuffle2(r["y"]), "y (pixel shuffle)")
        assert float(y[..., cout // 4:].float().abs().sum()) == 0.0, "pad channels of y"
    else:
        same(nchw64(y, cout), r["y"], "y")
        assert float(y[..., cout:].float().abs().sum()) == 0.0, "pad channels of y"
    if stats is not None:
        same(stats.double().sum(0)[:, :cout], r["stats"], "stats_partial (sum, sum of squares)")
    if dx is not None:
        same(nchw64(dx, c["cin"]), r["dx"], "dx")
        assert float(dx[..., c["cin"]:].float().abs().sum()) == 0.0, "pad channels of dx"
    if dw is not None:
        same(dw, r["dw"], "dw")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if not (c["stats"] or c["fold"] or c["residual"] or c["nchw"])])
def test_regime_a_conv_act(dev, name, dtype, monkeypatch):
    """The same layers through functional.ConvAct, forward and backward: y, dx, dw, db and the PReLU-slope gradient equal the
    reference, and functional.KERNEL_LOG records the kernels the case is there for."""
    F = P("functional")
    r = R.layer_a(name)
    c = r["case"]
    set_env(monkeypatch, c)
    log = []
    monkeypatch.setattr(F, "KERNEL_LOG", log)
    xg = nhwc(r["x"], dtype, dev).requires_grad_(c["dgrad"] is not None)
    wg = f32(r["w"], dev).requires_grad_(True)
    bg = f32(r["b"], dev).requires_grad_(True) if c["bias"] else None
    ag = torch.full((1,), c["slope"], device=dev, requires_grad=True) if c["act"] == R.ACT_PRELU else None
    cfg = dict(stride=c["stride"], pad=c["pad"], pad_mode=c["mode"], act=c["act"], slope=c["slope"], pixel_shuffle=c["ps"])
    if c["names"][2] is None:
        wg.requires_grad_(False)
    yg = F.ConvAct.apply(xg, wg, bg, ag, cfg)
    co = c["cout"] // 4 if c["ps"] else c["cout"]
    want_y, dy = (R.pixel_shuffle2(r["y"]), R.pixel_shuffle2(r["dy"])) if c["ps"] else (r["y"], r["dy"])
    if yg.requires_grad:
        yg.backward(nhwc(dy, dtype, dev, yg.shape[-1]))
    torch.cuda.synchronize()
    same(nchw64(yg.detach(), co), want_y, "y")
    assert float(yg.detach()[..., co:].float().abs().sum()) == 0.0, "pad channels of y"
    if c["dgrad"] is not None:
        same(nchw64(xg.grad, c["cin"]), r["dx_plain"], "dx")
        assert float(xg.grad[..., c["cin"]:].float().abs().sum()) == 0.0, "pad channels of dx"
    if c["names"][2] is not None:
        same(wg.grad, r["dw"], "dw")
        if bg is not None:
            same(bg.grad, r["db"], "db")
        if ag is not None:
            same(ag.grad, r["dprelu"].view(1), "dprelu")
    launched = {e[0]: e[4] for e in log}
    for kind, want in zip(("fwd", "dgrad", "wgrad"), c["names"]):
        if want is not None and not (kind == "dgrad" and c["dgrad"] is None):
            assert launched.get(kind) == want, (kind, launched, want)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["regime_b"]])
def test_regime_b_rounding(dev, name, dtype, monkeypatch):
    """Outputs beyond the representable integers (a few hundred exact ties among them, test_host_conv_exact.py): forward and
    input gradient must be the round-to-nearest-even image of the exact result -- truncation or a double rounding fails.

    Caught by t128_reflect_dma_128 (reflect-padded input gradient): dsr_conv_dgrad kept the gradient of the PADDED input in a
    16-bit workspace and reflect_fold_kernel rounded again after summing the mirrored entries, so 2641 (bf16) / 2676 (fp16) of
    63232 dx values, all on the two outermost rows and columns, were one unit off; the workspace is fp32 now."""
    L = P("_lib")
    lib = L.lib()
    r = R.layer_b(name, dtype)
    c = r["case"]
    set_env(monkeypatch, c)
    d = desc_of(L, c, dtype)
    wf, wd = pack(L, lib, d, r["w"], dtype, dev)
    can = Canaries(dev)
    y, _ = raw_forward(L, lib, dev, c, dtype, r, wf, can, plain=True)
    dx = raw_dgrad(L, lib, dev, c, dtype, r, r["g"], wd, can, "plain")
    can.check()
    same(nchw64(y, c["cout"]), r["y"], "y")
    same(nchw64(dx, c["cin"]), r["dx"], "dx")
    assert float(y[..., c["cout"]:].float().abs().sum()) == 0.0 and float(dx[..., c["cin"]:].float().abs().sum()) == 0.0


# ----------------------------------------------------------------------------- fused entry points outside the dispatcher
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (1, 70, 130)])
def test_dgrad_ps_exact(dev, n, h, w, dtype):
    """dsr_conv_dgrad_ps (9x9 tail input gradient + PixelShuffle-PReLU backward, slope 0.25): the masked, un-shuffled gradient,
    its column sums and the PReLU-slope gradient terms, all exact."""
    L = P("_lib")
    lib = L.lib()
    gen = torch.Generator().manual_seed(h * w)
    g3 = R.ternary(gen, (n, 3, h, w), 0.3)
    wt = R.ternary(gen, (3, 64, 9, 9), 0.3)
    out = R.small_ints(gen, (n, 64, h, w), 8)
    out = torch.where(out < 0, out * 0.25, out)                  # an activation OUTPUT: negatives are slope * integer
    dref = R.conv_dgrad(g3, wt, h, w, 1, 4, R.PAD_ZERO)
    gref = dref * R.act_grad_from_out(out, R.ACT_PRELU, 0.25)
    dyu_ref = R.pixel_unshuffle2(gref)
    dp_terms = dref * (out / 0.25) * (out < 0)
    assert R.representable(gref, dtype) and R.representable(out, dtype) and float(dp_terms.abs().sum()) < R.EXACT_LIMIT
    c = dict(n=n, h=h, w=w, cin=64, cout=3, k=9, stride=1, pad=4, mode=R.PAD_ZERO)
    d = desc_of(L, c, dtype)
    assert lib.dsr_conv_dgrad_ps_supported(C.byref(d)) == 1
    _, wd = pack(L, lib, d, wt, dtype, dev)
    can = Canaries(dev)
    rows = lib.dsr_conv_dgrad_ps_rows(C.byref(d))
    part = can.alloc((rows, 2, 256), torch.float32, "partial rows")
    dyu = can.alloc((n, h // 2, w // 2, 256), R.DTYPES[dtype], "dyu")
    gd, od = nhwc(g3, dtype, dev), nhwc(out, dtype, dev)
    prelu = torch.full((1,), 0.25, device=dev)
    L.check(lib.dsr_conv_dgrad_ps(C.byref(d), ptr(gd), ptr(wd), ptr(od), ptr(prelu), ptr(dyu), ptr(part), stream()))
    can.check()
    same(nchw64(dyu, 256), dyu_ref, "dyu")
    sums = part.double().sum(0).cpu()
    same(sums[0], dyu_ref.sum(dim=(0, 2, 3)), "bias-gradient column sums")
    same(sums[1].sum().view(1), dp_terms.sum().view(1), "PReLU-slope gradient")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,h,w,cin,cout,actn", [(2, 32, 32, 128, 128, "leaky"), (1, 4, 512, 64, 128, "none")])
def test_dgrad_bn_exact(dev, n, h, w, cin, cout, actn, dtype):
    """dsr_conv_dgrad_bn (3x3 stride-2 input gradient + the BatchNorm-backward sums of the layer in front) with a power-of-two
    scale, integer shift and LeakyReLU 0.25: dx and the partial rows summed per channel (sum g, sum g y, 0), all exact."""
    L = P("_lib")
    lib = L.lib()
    act = R.ACTS[actn]
    gen = torch.Generator().manual_seed(cin + h)
    g = R.ternary(gen, (n, cout, h // 2, w // 2), 0.3)
    wt = R.ternary(gen, (cout, cin, 3, 3), 0.3)
    y = R.small_ints(gen, (n, cin, h, w), 6)
    scale = 2.0 ** torch.randint(-1, 2, (cin,), generator=gen).double() * (torch.randint(0, 2, (cin,), generator=gen) * 2 - 1)
    shift = R.small_ints(gen, (cin,), 3)
    dx_ref = R.conv_dgrad(g, wt, h, w, 2, 1, R.PAD_ZERO)
    z = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    gg = dx_ref * (torch.where(z < 0, 0.25, 1.0) if act == R.ACT_LEAKY else 1.0)
    assert R.representable(dx_ref, dtype) and float((gg * y).abs().sum(dim=(0, 2, 3)).max()) < R.EXACT_LIMIT
    c = dict(n=n, h=h, w=w, cin=cin, cout=cout, k=3, stride=2, pad=1, mode=R.PAD_ZERO)
    d = desc_of(L, c, dtype)
    assert lib.dsr_conv_dgrad_bn_supported(C.byref(d)) == 1
    _, wd = pack(L, lib, d, wt, dtype, dev)
    can = Canaries(dev)
    rows = lib.dsr_conv_dgrad_bn_rows(C.byref(d))
    part = can.alloc((rows, 3, cin), torch.float32, "partial rows")
    dx = can.alloc((n, h, w, cin), R.DTYPES[dtype], "dx")
    gd, yd = nhwc(g, dtype, dev), nhwc(y, dtype, dev)
    sc, sh = f32(scale, dev), f32(shift, dev)
    L.check(lib.dsr_conv_dgrad_bn(C.byref(d), ptr(gd), ptr(wd), ptr(dx), ptr(yd), ptr(sc), ptr(sh), act, 0.25, ptr(part), stream()))
    can.check()
    same(nchw64(dx, cin), dx_ref, "dx")
    sums = part.double().sum(0).cpu()
    same(sums[0], gg.sum(dim=(0, 2, 3)), "sum g")
    same(sums[1], (gg * y).sum(dim=(0, 2, 3)), "sum g y")
    assert float(sums[2].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DT)
def test_wgrad_batched_exact(dev, dtype):
    """dsr_conv_wgrad_batched with three layers, two of which share dw (their gradients are summed): exact."""
    L = P("_lib")
    lib = L.lib()
    gen = torch.Generator().manual_seed(31)
    shapes = [(2, 24, 40, 64, 64, R.PAD_ZERO), (1, 17, 33, 64, 128, R.PAD_ZERO), (2, 17, 33, 64, 128, R.PAD_ZERO)]
    can = Canaries(dev)
    dws = [can.alloc((64, 64, 3, 3), torch.float32, "dw 0"), can.alloc((128, 64, 3, 3), torch.float32, "dw 1")]
    dws.append(dws[1])
    refs = [torch.zeros(64, 64, 3, 3, dtype=torch.float64), torch.zeros(128, 64, 3, 3, dtype=torch.float64)]
    descs, xs, gs = [], [], []
    for i, (n, h, w, cin, cout, pm) in enumerate(shapes):
        x, g = R.ternary(gen, (n, cin, h, w), 0.3), R.ternary(gen, (n, cout, h, w), 0.3)
        refs[min(i, 1)] += R.conv_wgrad(x, g, 3, 1, 1, pm)
        descs.append(L.ConvDesc(dtype, n, h, w, cin, cout, 3, 3, 1, 1, pm))
        xs.append(nhwc(x, dtype, dev))
        gs.append(nhwc(g, dtype, dev))
    darr = (L.ConvDesc * 3)(*descs)
    xa, ga, wa = ((C.c_void_p * 3)(*[t.data_ptr() for t in ts]) for ts in (xs, gs, dws))
    wsz = lib.dsr_conv_wgrad_batched_workspace(3, darr, wa)
    assert wsz > 0
    ws = can.alloc((wsz,), torch.uint8, "workspace")
    L.check(lib.dsr_conv_wgrad_batched(3, darr, xa, ga, wa, ptr(ws), wsz, stream()))
    can.check()
    same(dws[0], refs[0], "dw 0")
    same(dws[1], refs[1], "dw 1 (two batches summed)")


def _first_layer_operands(dtype, n, h, w, cin):
    """Image layer 3 -> 64 with operands whose pre-activation is never zero (even products, odd integer bias): the stored-output
    and the recomputed-sign forms of the first-layer backward then agree on every branch."""
    gen = torch.Generator().manual_seed(17 * h + w + cin)
    x = 2 * R.ternary(gen, (n, cin, h, w), 0.3)
    w0 = R.ternary(gen, (64, cin, 3, 3), 0.3)
    b0 = 2 * R.small_ints(gen, (64,), 2) + 1
    z0 = R.conv_fwd(x, w0, 1, 1, R.PAD_ZERO) + b0.view(1, -1, 1, 1)
    assert int((z0 == 0).sum()) == 0 and int((z0 < 0).sum()) > 100
    a0 = R.act_fwd(z0, R.ACT_LEAKY, 0.25)
    assert R.representable(a0, dtype)
    return gen, x, w0, b0, a0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("recompute", [False, True], ids=["stored_output", "recompute"])
def test_first_bwd_exact(dev, recompute, dtype):
    """dsr_conv_first_bwd / _recompute (3 -> 64 3x3 + LeakyReLU 0.25, no input gradient): dw and db in one pass, exact."""
    L = P("_lib")
    lib = L.lib()
    n, h, w, cin = 2, 19, 37, 3
    gen, x, w0, b0, a0 = _first_layer_operands(dtype, n, h, w, cin)
    dout = R.ternary(gen, (n, 64, h, w), 0.4)
    g = dout * R.act_grad_from_out(a0, R.ACT_LEAKY, 0.25)
    dw_ref, db_ref = R.conv_wgrad(x, g, 3, 1, 1, R.PAD_ZERO), g.sum(dim=(0, 2, 3))
    d = L.ConvDesc(dtype, n, h, w, cin, 64, 3, 3, 1, 1, R.PAD_ZERO)
    assert lib.dsr_conv_first_bwd_supported(C.byref(d), R.ACT_LEAKY) == 1
    can = Canaries(dev)
    dw, db = can.alloc((64, cin, 3, 3), torch.float32, "dw"), can.alloc((64,), torch.float32, "db")
    wsz = lib.dsr_conv_first_bwd_workspace(C.byref(d))
    ws = can.alloc((wsz,), torch.uint8, "workspace")
    xd, dd, yd = nhwc(x, dtype, dev), nhwc(dout, dtype, dev), nhwc(a0, dtype, dev)
    if recompute:
        wdev, bdev = f32(w0, dev), f32(b0, dev)
        L.check(lib.dsr_conv_first_bwd_recompute(C.byref(d), ptr(xd), ptr(dd), ptr(wdev), ptr(bdev), R.ACT_LEAKY, 0.25, ptr(dw), ptr(db),
                                                 ptr(ws), wsz, stream()))
    else:
        L.check(lib.dsr_conv_first_bwd(C.byref(d), ptr(xd), ptr(dd), ptr(yd), R.ACT_LEAKY, 0.25, ptr(dw), ptr(db), ptr(ws), wsz,
                                       stream()))
    can.check()
    same(dw, dw_ref, "dw")
    same(db, db_ref, "db")


@pytest.mark.parametrize("dtype", DT)
def test_first2_fwd_exact(dev, dtype):
    """dsr_conv_first2_fwd (3 -> 64 3x3 + LeakyReLU 0.25, then 64 -> 64 3x3 stride 2, one launch; integer biases: they ride as a
    16-bit column): the stored first activation, the second layer's raw output and its statistics rows, exact."""
    L = P("_lib")
    lib = L.lib()
    n, h, w, cin = 2, 19, 37, 3
    gen, x, w0, b0, a0 = _first_layer_operands(dtype, n, h, w, cin)
    w1 = R.ternary(gen, (64, 64, 3, 3), 0.02)
    b1 = R.small_ints(gen, (64,), 3)
    y1 = R.conv_fwd(a0, w1, 2, 1, R.PAD_ZERO) + b1.view(1, -1, 1, 1)
    assert R.representable(y1, dtype) and float((y1 * y1).sum(dim=(0, 2, 3)).max()) * 16 < R.EXACT_LIMIT
    d0 = L.ConvDesc(dtype, n, h, w, cin, 64, 3, 3, 1, 1, R.PAD_ZERO)
    d1 = L.ConvDesc(dtype, n, h, w, 64, 64, 3, 3, 2, 1, R.PAD_ZERO)
    assert lib.dsr_conv_first2_supported(C.byref(d0), C.byref(d1)) == 1
    wf0, _ = pack(L, lib, d0, w0, dtype, dev)
    wf1, _ = pack(L, lib, d1, w1, dtype, dev)
    oh, ow = R.out_size(h, w, 3, 2, 1)
    can = Canaries(dev)
    a0g = can.alloc((n, h, w, 64), R.DTYPES[dtype], "a0")
    y1g = can.alloc((n, oh, ow, 64), R.DTYPES[dtype], "y1")
    rows = lib.dsr_conv_first2_stats_rows(C.byref(d0))
    st = can.alloc((rows, 2, 64), torch.float32, "stats rows")
    xd, b0d, b1d = nhwc(x, dtype, dev), f32(b0, dev), f32(b1, dev)
    L.check(lib.dsr_conv_first2_fwd(C.byref(d0), C.byref(d1), ptr(xd), ptr(wf0), ptr(b0d), 0.25, ptr(wf1), ptr(b1d), ptr(a0g), ptr(y1g),
                                    ptr(st), stream()))
    can.check()
    same(nchw64(a0g, 64), a0, "a0")
    same(nchw64(y1g, 64), y1, "y1")
    same(st.double().sum(0), torch.stack([y1.sum(dim=(0, 2, 3)), (y1 * y1).sum(dim=(0, 2, 3))]), "stats rows")


@pytest.mark.parametrize("dtype", DT)
def test_dgrad_first_bwd_exact(dev, dtype):
    """dsr_conv_dgrad_first_bwd (input gradient of the 64 -> 64 3x3 stride-2 layer + the whole backward of the 3 -> 64 image
    layer with LeakyReLU 0.25 under it, one launch; conv_dgrad_s2_kernel's first-layer instantiation, whose bias column is the
    storage type's own 1.0): dw0 and db0 by equality.  The gradient of the activation in between is never written, so there
    is no dx to compare.  Two rows of tiles (W / 2 = 256 gradient pixels per tile), all four image borders."""
    L = P("_lib")
    lib = L.lib()
    n, h, w, cin = 2, 6, 512, 3
    gen, x, w0, b0, a0 = _first_layer_operands(dtype, n, h, w, cin)
    w1 = R.ternary(gen, (64, 64, 3, 3), 0.2)
    dy = R.ternary(gen, (n, 64, h // 2, w // 2), 0.3)
    da0 = R.conv_dgrad(dy, w1, h, w, 2, 1, R.PAD_ZERO)
    g0 = da0 * R.act_grad_from_out(a0, R.ACT_LEAKY, 0.25)        # (the pre-activation is never zero: a0's sign is its sign)
    assert R.representable(da0, dtype) and R.representable(g0, dtype) and int((g0 != 0).sum()) > g0.numel() // 4
    dw_ref, db_ref = R.conv_wgrad(x, g0, 3, 1, 1, R.PAD_ZERO), g0.sum(dim=(0, 2, 3))
    assert float(R.conv_wgrad(x.abs(), g0.abs(), 3, 1, 1, R.PAD_ZERO).max()) < R.EXACT_LIMIT
    d0 = L.ConvDesc(dtype, n, h, w, cin, 64, 3, 3, 1, 1, R.PAD_ZERO)
    d1 = L.ConvDesc(dtype, n, h, w, 64, 64, 3, 3, 2, 1, R.PAD_ZERO)
    assert lib.dsr_conv_dgrad_first_bwd_supported(C.byref(d0), C.byref(d1), R.ACT_LEAKY) == 1
    _, wd1 = pack(L, lib, d1, w1, dtype, dev)
    can = Canaries(dev)
    dw, db = can.alloc((64, cin, 3, 3), torch.float32, "dw0"), can.alloc((64,), torch.float32, "db0")
    wsz = lib.dsr_conv_dgrad_first_bwd_workspace(C.byref(d1))
    ws = can.alloc((wsz,), torch.uint8, "workspace")
    xd, dyd, w0d, b0d = nhwc(x, dtype, dev), nhwc(dy, dtype, dev), f32(w0, dev), f32(b0, dev)
    L.check(lib.dsr_conv_dgrad_first_bwd(C.byref(d0), C.byref(d1), ptr(dyd), ptr(wd1), ptr(xd), ptr(w0d), ptr(b0d), R.ACT_LEAKY, 0.25,
                                         ptr(dw), ptr(db), ptr(ws), wsz, stream()))
    can.check()
    same(dw, dw_ref, "dw0")
    same(db, db_ref, "db0")
