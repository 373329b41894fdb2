"""GPU: float64 / exact-integer parity sweep of the pointwise BatchNorm family of csrc/pointwise.hip, in bf16 and fp16
(reference and case table: pointwise_ref.py; regime proofs, thresholds and argument checks: test_host_pointwise.py).

Exact regime: small-integer data and power-of-two parameters make every product and partial sum exact in fp32 and every stored
value representable, so each 16-bit output and each partial row must EQUAL the float64 reference, whichever instantiation
(compile-time activation or run-time fallback, cached or non-temporal, parallel or serial finalize) produced it.  Rounded
regime: real-valued data, large-mean channels included, against bounds derived from the arithmetic (stated at each check), never
measured on the kernels.  Every output and partial buffer of a raw C-ABI call sits inside a sentinel-filled buffer whose margins
must come back untouched; partial buffers carry the dsr_pw_scratch_rows() extra rows the product allocates, in front of the
margin."""
import ctypes as C
import importlib
import math

import pytest
import torch

import pointwise_ref as R
from canaries import Canaries

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
EPS, MOMENTUM = 1e-5, 0.1
U24 = 2.0 ** -24      # half an fp32 ulp, relative: the error of one fp32 rounding


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


def up16(t, dtype, dev):
    """float64 -> the 16-bit storage type on the device; the values must be representable."""
    out = t.to(R.DTYPES[dtype])
    assert torch.equal(out.to(torch.float64), t.to(torch.float64))
    return out.contiguous().to(dev)


def f32(t, dev):
    if t is None:
        return None
    out = t.to(torch.float32)
    assert torch.equal(out.to(torch.float64), t.to(torch.float64)), "parameter not exact in fp32"
    return out.contiguous().to(dev)


def same(got, want, what):
    """Numeric equality (-0 equals +0; NaN equals NaN), on whichever device `got` lives, with the first differing positions."""
    got, want = got.to(torch.float64), want.to(torch.float64).to(got.device)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = ((got != want) & ~(got.isnan() & want.isnan())).nonzero()
        if len(bad):
            raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ; first at {bad[:6].tolist()}: got "
                                 f"{got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")


def within(got, ref, bound, what, allow=None):
    got, ref = got.to(torch.float64).cpu(), ref.to(torch.float64)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if allow is not None:
        bad &= ~allow
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        ratio = torch.where(bad, err / (bound + torch.zeros_like(err)).clamp_min(1e-300), torch.zeros_like(err))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} beyond the bound; first at {list(i)}: got {got[i].item()!r} "
                             f"ref {ref[i].item()!r} err {err[i].item():.3e} bound {(bound + torch.zeros_like(err))[i].item():.3e}; "
                             f"largest err / bound {float(ratio.max()):.3f}")


def neighbour(got, ref, dtype, what, allow=None):
    """The 16-bit result is one of the two values of the storage type that enclose the float64 reference (<= 1 ulp)."""
    got, ref = got.to(torch.float64).cpu(), ref.to(torch.float64)
    a, b = R.neighbours(ref, dtype)
    bad = ~((got == a) | (got == b))
    if allow is not None:
        bad &= ~allow
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} are no neighbour of the reference; first at {list(i)}: got "
                             f"{got[i].item()!r} ref {ref[i].item()!r} neighbours {a[i].item()!r} {b[i].item()!r}; largest "
                             f"|err| / ulp {float(((got - ref).abs() / R.ulp16(ref, dtype)).max()):.3f}")


# ----------------------------------------------------------------------------- the entry points, into canary buffers
class Calls:
    def __init__(self, dev, dtype):
        self.L = P("_lib")
        self.lib = self.L.lib()
        self.dev, self.dtype, self.tdt = dev, dtype, R.DTYPES[dtype]
        self.can = Canaries(dev)
        self.keep = []

    def rows(self, blocks, k, cp, what):
        """A partial buffer of `blocks` rows [k][cp] with the scratch rows the product allocates behind them."""
        full = self.can.alloc((blocks + R.SCRATCH_ROWS, k, cp), torch.float32, what)
        return full, full[:blocks]

    def slope_args(self, act, slope):
        if act == R.ACT_PRELU:
            w = torch.full((1,), slope, dtype=torch.float32, device=self.dev)
            self.keep.append(w)
            return 0.0, ptr(w)
        return float(slope), None

    def channel_stats(self, x, p, cp, rpb):
        blocks = R.n_blocks(p, rpb)
        full, part = self.rows(blocks, 2, cp, "channel_stats partial")
        self.L.check(self.lib.dsr_pw_channel_stats(self.dtype, ptr(x), p, cp, blocks, rpb, ptr(full), stream()))
        return full, part

    def colsum(self, x, p, cp, rpb):
        blocks = R.n_blocks(p, rpb)
        full, part = self.rows(blocks, 1, cp, "colsum partial")
        self.L.check(self.lib.dsr_pw_colsum(self.dtype, ptr(x), p, cp, blocks, rpb, ptr(full), stream()))
        return part

    def bn_act_fwd(self, y, scale, shift, residual, p, cp, act, slope):
        out = self.can.alloc((p, cp), self.tdt, "bn_act_fwd out")
        sv, pw = self.slope_args(act, slope)
        self.L.check(self.lib.dsr_pw_bn_act_fwd(self.dtype, ptr(y), ptr(scale), ptr(shift), ptr(residual), ptr(out), p, cp, act, sv, pw,
                                                stream()))
        return out

    def bwd_reduce(self, dout, y, scale, shift, mean, rstd, p, cp, rpb, act, slope):
        blocks = R.n_blocks(p, rpb)
        full, part = self.rows(blocks, 3, cp, "bn_act_bwd_reduce partial")
        sv, pw = self.slope_args(act, slope)
        self.L.check(self.lib.dsr_pw_bn_act_bwd_reduce(self.dtype, ptr(dout), ptr(y), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), p, cp,
                                                       blocks, rpb, act, sv, pw, ptr(full), stream()))
        return full, part

    def bwd_apply(self, dout, y, scale, shift, mean, rstd, c1, c2, p, cp, act, slope, train):
        dy = self.can.alloc((p, cp), self.tdt, "bn_act_bwd_apply dy")
        sv, pw = self.slope_args(act, slope)
        self.L.check(self.lib.dsr_pw_bn_act_bwd_apply(self.dtype, ptr(dout), ptr(y), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(c1),
                                                      ptr(c2), ptr(dy), p, cp, act, sv, pw, int(train), stream()))
        return dy

    def act_bwd(self, dout, out, n, h, w, cyp, cop, pixshuf, act, slope, rpb, expect=0):
        p = n * h * w
        blocks = R.n_blocks(p, rpb)
        dy = self.can.alloc((p, cyp), self.tdt, "act_bwd dy")
        full, part = self.rows(blocks, 2, cyp, "act_bwd partial")
        sv, pw = self.slope_args(act, slope)
        rc = self.lib.dsr_pw_act_bwd(self.dtype, ptr(dout), ptr(out), ptr(dy), n, h, w, cyp, cop, int(pixshuf), act, sv, pw, blocks, rpb,
                                     ptr(full), stream())
        assert rc == expect, (rc, self.lib.dsr_last_error())
        return dy, part, full

    def bn_finalize(self, full, rows, stride, c, cp, count, gamma, beta, rm, rv, nbt, updates):
        outs = [self.can.alloc((cp,), torch.float32, "bn_finalize " + k) for k in ("scale", "shift", "mean", "rstd")]
        self.L.check(self.lib.dsr_pw_bn_finalize(ptr(full), rows, stride, c, cp, float(count), ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                                                 ptr(nbt), MOMENTUM, EPS, updates, *[ptr(o) for o in outs], stream()))
        return dict(zip(("scale", "shift", "mean", "rstd"), outs))

    def bn_bwd_finalize(self, full, rows, c, cp, count, mean, rstd, with_prelu=True):
        o = dict(dgamma=self.can.alloc((c,), torch.float32, "dgamma"), dbeta=self.can.alloc((c,), torch.float32, "dbeta"),
                 dprelu=self.can.alloc((1,), torch.float32, "dprelu") if with_prelu else None,
                 c1=self.can.alloc((cp,), torch.float32, "c1"), c2=self.can.alloc((cp,), torch.float32, "c2"))
        self.L.check(self.lib.dsr_pw_bn_bwd_finalize(ptr(full), rows, c, cp, float(count), ptr(mean), ptr(rstd), ptr(o["dgamma"]),
                                                     ptr(o["dbeta"]), ptr(o["dprelu"]), ptr(o["c1"]), ptr(o["c2"]), stream()))
        return o


def chain_k(rpb, rpi):
    """Longest fp32 addition chain of the documented summation tree of a block's partial row: ceil(rpb / rpi) additions in a
    thread, rpi across the block's threads, and two roundings inside a term (its product and, in the backward, g itself)."""
    return math.ceil(rpb / rpi) + rpi + 2


# ----------------------------------------------------------------------------- exact regime: the streaming family
def exact_family(k, d, dev, dtype, acts, ref_dev="cpu"):
    """Every row-walking kernel on the exact-regime operands d (float64, on ref_dev): results == reference."""
    case = d["case"]
    p, cp, c, rpb = case["p"], case["cp"], case["c"], case["rpb"]
    y, dout, res = (up16(d[q], dtype, dev) for q in ("y", "dout", "residual"))
    par = {q: f32(d[q], dev) for q in ("scale", "shift", "mean", "rstd", "c1", "c2")}
    todo = []
    _, got = k.channel_stats(y, p, cp, rpb)
    todo.append((got, R.channel_stats(d["y"], rpb), "channel_stats"))
    todo.append((k.colsum(dout, p, cp, rpb), R.colsum(d["dout"], rpb), "colsum"))
    for i, (act, slope) in enumerate(acts):
        tag = f"{R.ACT_NAMES[act]}({slope})"
        use_res = i % 2 == 0
        got = k.bn_act_fwd(y, par["scale"], par["shift"], res if use_res else None, p, cp, act, slope)
        todo.append((got, R.bn_act_fwd(d["y"], d["scale"], d["shift"], d["residual"] if use_res else None, act, slope), "bn_act_fwd " + tag))
        if i == 0 or act == R.ACT_PRELU:      # the identity form: out = act(y) + residual
            got = k.bn_act_fwd(y, None, None, res, p, cp, act, slope)
            todo.append((got, R.bn_act_fwd(d["y"], None, None, d["residual"], act, slope), "bn_act_fwd identity " + tag))
        _, got = k.bwd_reduce(dout, y, par["scale"], par["shift"], par["mean"], par["rstd"], p, cp, rpb, act, slope)
        todo.append((got, R.bn_act_bwd_reduce(d["dout"], d["y"], d["scale"], d["shift"], act, slope, rpb), "bn_act_bwd_reduce " + tag))
        for train in (True, False):
            got = k.bwd_apply(dout, y, par["scale"], par["shift"], par["mean"], par["rstd"], par["c1"], par["c2"], p, cp, act, slope, train)
            want = R.bn_act_bwd_apply(d["dout"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["c1"], d["c2"], act, slope, train)
            todo.append((got, want, f"bn_act_bwd_apply train={train} " + tag))
        # act_bwd reads the stored activation output: the forward's own (no residual), which the host test shows representable
        o64 = R.bn_act_fwd(d["y"], d["scale"], d["shift"], None, act, slope)
        dy, part, _ = k.act_bwd(dout, up16(o64, dtype, dev), 1, 1, p, cp, cp, False, act, slope, rpb)
        wdy, wpart = R.act_bwd(d["dout"], o64, act, slope, rpb)
        todo += [(dy, wdy, "act_bwd dy " + tag), (part, wpart, "act_bwd partial " + tag)]
    k.can.check()
    for got, want, what in todo:
        same(got if ref_dev != "cpu" else got.cpu(), want, f"{case['name']} {what}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.STREAM_IDS)
def test_exact_stream_family(dev, name, dtype):
    """channel_stats, colsum, bn_act_fwd (affine + residual, and the scale == NULL identity form), bn_act_bwd_reduce (three
    slices), bn_act_bwd_apply (train and eval) and act_bwd (dy and both partial slices), for none / ReLU / LeakyReLU / PReLU at
    two slopes: bit equality with the float64 reference at every thread mapping (Cp 8 .. 2048) and row count (1, rpi - 1,
    rpi + 1, 2 rpi + 1, a prime with a short last block); canary margins intact."""
    exact_family(Calls(dev, dtype), R.exact_stream_cpu(name), dev, dtype, R.EXACT_ACTS)


@pytest.mark.parametrize("dtype", DT)
def test_exact_capped_grid(dev, dtype):
    """Cp = 64, P = 4096 * 32 * 2 + 33: the streaming kernels' grid is capped at 4096 blocks, so the stride loop iterates and the
    tail executes; the reductions run on the grid dsr_pw_reduce_blocks gives.  Data and float64 reference on the device."""
    k = Calls(dev, dtype)
    rpb = C.c_int(0)
    blocks = k.lib.dsr_pw_reduce_blocks(R.CAPPED["p"], C.byref(rpb))
    assert blocks == R.n_blocks(R.CAPPED["p"], rpb.value) and R.CAPPED["p"] % rpb.value
    d = R.exact_stream(dict(R.CAPPED, rpb=rpb.value), device=dev)
    exact_family(k, d, dev, dtype, [(R.ACT_PRELU, 0.25), (R.ACT_LEAKY, 0.25)], ref_dev=dev)


NT_KERNELS = ["bn_act_fwd", "bn_act_bwd_reduce", "bn_act_bwd_apply", "act_bwd"]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel", NT_KERNELS)
def test_exact_nontemporal(dev, kernel, dtype):
    """Cp = 64, P = 6 * 512 * 512 + 1: just over the 192 MiB from which the launchers pick the non-temporal instantiation (the
    size is the only way in; the environment override is read once per process and is not touched).  Exact regime, data and
    float64 reference on the device."""
    case = R.NONTEMPORAL
    p, cp = case["p"], case["cp"]
    assert p * cp * 2 >= R.NT_BYTES
    k = Calls(dev, dtype)
    rpb = C.c_int(0)
    k.lib.dsr_pw_reduce_blocks(p, C.byref(rpb))
    rpb = rpb.value
    gen = torch.Generator(device=dev).manual_seed(11 + dtype)
    draw = lambda: torch.randint(-3, 4, (p, cp), generator=gen, device=dev, dtype=torch.int8).to(k.tdt)
    par64 = R.exact_stream(dict(case, p=1, rpb=1, name="nt_params"), device=dev)
    par = {q: f32(par64[q], dev) for q in ("scale", "shift", "mean", "rstd", "c1", "c2")}
    sc, sh = par64["scale"], par64["shift"]
    act, slope = R.ACT_PRELU, 0.25
    y, dout = draw(), draw()
    if kernel == "bn_act_fwd":
        res = draw()
        got = k.bn_act_fwd(y, par["scale"], par["shift"], res, p, cp, act, slope)
        k.can.check()
        want = R.bn_act_fwd(y.double(), sc, sh, res.double(), act, slope)
        same(got, want, "bn_act_fwd")
    elif kernel == "bn_act_bwd_reduce":
        _, got = k.bwd_reduce(dout, y, par["scale"], par["shift"], par["mean"], par["rstd"], p, cp, rpb, act, slope)
        k.can.check()
        same(got, R.bn_act_bwd_reduce(dout.double(), y.double(), sc, sh, act, slope, rpb), "bn_act_bwd_reduce")
    elif kernel == "bn_act_bwd_apply":
        got = k.bwd_apply(dout, y, par["scale"], par["shift"], par["mean"], par["rstd"], par["c1"], par["c2"], p, cp, act, slope, True)
        k.can.check()
        want = R.bn_act_bwd_apply(dout.double(), y.double(), sc, sh, par64["mean"], par64["rstd"], par64["c1"], par64["c2"], act, slope, True)
        same(got, want, "bn_act_bwd_apply")
    else:
        out = torch.where(y >= 0, y, y * slope)          # a stored PReLU output: integers, or quarter-integers below zero
        dy, part, _ = k.act_bwd(dout, out, 1, 1, p, cp, cp, False, act, slope, rpb)
        k.can.check()
        wdy, wpart = R.act_bwd(dout.double(), out.double(), act, slope, rpb)
        same(dy, wdy, "act_bwd dy")
        same(part, wpart, "act_bwd partial")


@pytest.mark.parametrize("dtype", DT)
def test_exact_act_bwd_pixel_unshuffle(dev, dtype):
    """act_bwd with pixshuf = 1: dy[n, h, w, 4c + 2i + j] from pixel (2h + i, 2w + j) of channel c, with and without padded
    shuffle channels (CyP != 4 CoP), several blocks with a short last one; dy and both partial slices equal the reference."""
    k = Calls(dev, dtype)
    todo = []
    for n, h, w, c in R.PIXSHUF_CASES:
        cop, cyp = R.r8(c), R.r8(4 * c)
        gen = torch.Generator().manual_seed(100 * c + h)
        p = n * h * w
        rpb = max(1, p // 3)
        for act, slope in R.EXACT_ACTS[1:]:
            out = R.exact_act_out(gen, (n, 2 * h, 2 * w, cop), c, slope)
            dout = R.ints(gen, (n, 2 * h, 2 * w, cop), 3)
            dout[..., c:] = 0
            dy, part, _ = k.act_bwd(up16(dout, dtype, dev), up16(out, dtype, dev), n, h, w, cyp, cop, True, act, slope, rpb)
            wdy, wpart = R.act_bwd(R.unshuffle_nhwc(dout, cyp).reshape(p, cyp), R.unshuffle_nhwc(out, cyp).reshape(p, cyp), act, slope, rpb)
            assert float(wdy[:, 4 * c:].abs().sum()) == 0.0
            todo += [(dy, wdy, f"dy {(n, h, w, c)} {R.ACT_NAMES[act]}"), (part, wpart, f"partial {(n, h, w, c)} {R.ACT_NAMES[act]}")]
    k.can.check()
    for got, want, what in todo:
        same(got.cpu(), want, what)


@pytest.mark.parametrize("dtype", DT)
def test_act_bwd_slope_checks(dev, dtype):
    """A PReLU slope of 0 or -0.25 on the device turns dy and both partial slices into NaN (never a silently wrong gradient); a
    LeakyReLU slope <= 0 is rejected with an error and launches nothing (the outputs keep their fill)."""
    k = Calls(dev, dtype)
    d = R.exact_stream_cpu("cp24_p997_rpb100")
    p, cp = d["case"]["p"], d["case"]["cp"]
    dout, out = up16(d["dout"], dtype, dev), up16(d["y"], dtype, dev)
    res = [k.act_bwd(dout, out, 1, 1, p, cp, cp, False, R.ACT_PRELU, s, 100) for s in (0.0, -0.25)]
    rej = [k.act_bwd(dout, out, 1, 1, p, cp, cp, False, R.ACT_LEAKY, s, 100, expect=-1) for s in (0.0, -0.25)]
    k.can.check()
    for dy, part, _ in res:
        assert bool(dy.isnan().all()) and bool(part.isnan().all())
    for dy, _, full in rej:
        assert k.can.untouched(dy) and k.can.untouched(full)


@pytest.mark.parametrize("dtype", DT)
def test_act_bwd_nchw_and_add(dev, dtype):
    """act_bwd_nchw (fp32 NCHW dout / out -> 16-bit NHWC dy, zero pad channels): equality for integer dout without activation, one
    of the two neighbours of the float64 value for tanh / sigmoid.  add: equality on integers, a neighbour on real data."""
    k = Calls(dev, dtype)
    gen = torch.Generator().manual_seed(17)
    todo = []
    for n, c, h, w, act in R.NCHW_CASES:
        cp = R.r8(c)
        if act == R.ACT_NONE:
            dout, out = R.ints(gen, (n, c, h, w), 3), R.ints(gen, (n, c, h, w), 3)
        else:
            dout = torch.randn(n, c, h, w, generator=gen).double()
            # |z| of a few units: 1 - o^2 is read off the fp32 OUTPUT by contract, and stays well conditioned there
            out = R.act_fwd(torch.randn(n, c, h, w, generator=gen, dtype=torch.float64), act).float().double()
        dy = k.can.alloc((n, h, w, cp), k.tdt, "act_bwd_nchw dy")
        k.keep += [f32(dout, dev), f32(out, dev)]
        k.L.check(k.lib.dsr_pw_act_bwd_nchw(dtype, ptr(k.keep[-2]), ptr(k.keep[-1]), ptr(dy), n, c, h, w, cp, act, stream()))
        todo.append((dy, R.act_bwd_nchw(dout, out, act, cp), act == R.ACT_NONE, f"act_bwd_nchw {(n, c, h, w)}"))
    for nvec in R.ADD_NVEC:
        for exact in (True, False):
            a, b = ((R.ints(gen, (nvec * 8,), 60), R.ints(gen, (nvec * 8,), 60)) if exact else
                    (R.r16(torch.randn(nvec * 8, generator=gen, dtype=torch.float64) * 3, dtype) for _ in range(2)))
            out = k.can.alloc((nvec * 8,), k.tdt, "add out")
            k.keep += [up16(a, dtype, dev), up16(b, dtype, dev)]
            k.L.check(k.lib.dsr_pw_add(dtype, ptr(k.keep[-2]), ptr(k.keep[-1]), ptr(out), nvec, stream()))
            todo.append((out, R.add(a, b), exact, f"add nvec={nvec}"))
    k.can.check()
    for got, want, exact, what in todo:
        if exact:
            same(got.cpu(), want, what)
        else:
            neighbour(got, want, dtype, what)


# ----------------------------------------------------------------------------- the finalize kernels
@pytest.mark.parametrize("rows,cp,stride,updates", R.FINALIZE_CASES, ids=["rows%d_cp%d_stride%d" % c[:3] for c in R.FINALIZE_CASES])
def test_bn_finalize(dev, rows, cp, stride, updates):
    """Exact (integer) partial rows on every side of the launcher's thresholds -- serial, parallel <64> and <16>, compaction to 16
    and to 64 chunks, stride > Cp.  The sums are exact in the kernel's fp64, so what is left is: mean = one rounding of a float64
    quotient; rstd = one rounding of a float64 expression; scale = rstd * gamma, one more; each running statistic 3 roundings per
    update on top of those -- all inside 4 fp32 ulp of the float64 value.  shift = beta - mean * scale: 4 * 2^-24 * (|beta| +
    |mean * scale|).  num_batches exact; the pad channels of all four outputs exactly 0.0; scratch rows and margins respected."""
    k = Calls(dev, R.BF16)
    c = R.C_OF_CP[cp]
    part = R.finalize_rows(rows, cp, stride, c)
    gen = torch.Generator().manual_seed(rows + cp)
    gamma = (0.5 + torch.rand(c, generator=gen)).double()
    beta = torch.randn(c, generator=gen).double()
    full = k.can.alloc((rows + R.SCRATCH_ROWS, 2, stride), torch.float32, "bn_finalize partial")
    if rows == 4200:
        # the rows as channel_stats itself writes them: one pixel per row (P = 4200, rpb = 1), pad columns zero
        x = torch.zeros(rows, cp, dtype=torch.float64)
        x[:, :c] = part[:, 0, :c]
        part = R.channel_stats(x, 1)
        k.L.check(k.lib.dsr_pw_channel_stats(R.BF16, ptr(up16(x, R.BF16, dev)), rows, cp, rows, 1, ptr(full), stream()))
        torch.cuda.synchronize()
        same(full[:rows].cpu(), part, "channel_stats rows (rpb = 1)")
    else:
        full[:rows] = f32(part, dev)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    nbt = torch.full((1,), 41, dtype=torch.int64, device=dev)
    got = k.bn_finalize(full, rows, stride, c, cp, rows, f32(gamma, dev), f32(beta, dev), rm, rv, nbt, updates)
    k.can.check()
    want = R.bn_finalize(part, c, cp, float(rows), gamma, beta, torch.zeros(c), torch.ones(c), 41, MOMENTUM, EPS, updates)
    assert int(nbt.item()) == want["num_batches"] == 41 + updates
    for key in ("mean", "rstd", "scale", "shift"):
        assert float(got[key][c:].abs().sum()) == 0.0 and not bool(got[key].isnan().any()), f"pad channels of {key}"
    for key in ("mean", "rstd", "scale"):
        within(got[key], want[key], 4 * R.ulp32(want[key]), key)
    within(got["shift"][:c], want["shift"][:c], 4 * U24 * (beta.abs() + (want["mean"] * want["scale"])[:c].abs()), "shift")
    within(rm, want["running_mean"], 4 * R.ulp32(want["running_mean"]), "running_mean")
    within(rv, want["running_var"], 4 * R.ulp32(want["running_var"]), "running_var")
    assert torch.equal(full[:rows].cpu().double(), part), "the partial rows themselves were modified"


@pytest.mark.parametrize("rows,cp,with_prelu", R.BWD_FINALIZE_CASES,
                         ids=["rows%d_cp%d_%s" % (r, cp, "dprelu" if w else "nodprelu") for r, cp, w in R.BWD_FINALIZE_CASES])
def test_exact_bn_bwd_finalize(dev, rows, cp, with_prelu):
    """Integer partial rows, integer mean, power-of-two rstd and count: dgamma = rstd (sum g*y - mean sum g), dbeta, dprelu (real
    channels only: the pad columns hold junk), c1 and c2 (pad channels 0) equal the reference on both sides of every threshold
    -- serial, parallel, compaction -- with and without dprelu, Cp > 64 with dprelu forcing the single-block kernel."""
    k = Calls(dev, R.BF16)
    c = R.C_OF_CP[cp]
    part, mean, rstd = R.bwd_finalize_rows(rows, cp, c)
    full = k.can.alloc((rows + R.SCRATCH_ROWS, 3, cp), torch.float32, "bn_bwd_finalize partial")
    full[:rows] = f32(part, dev)
    got = k.bn_bwd_finalize(full, rows, c, cp, 64.0, f32(mean, dev), f32(rstd, dev), with_prelu)
    k.can.check()
    want = R.bn_bwd_finalize(part, c, cp, 64.0, mean, rstd)
    for key in ("dgamma", "dbeta", "c1", "c2"):
        same(got[key].cpu(), want[key], key)
    if with_prelu:
        same(got["dprelu"].cpu(), want["dprelu"].reshape(1), "dprelu")


@pytest.mark.parametrize("rows,stride,off,c,compact,accumulate,scale", R.SUM_ROWS_CASES,
                         ids=["rows%d_stride%d_c%d_a%d" % (r, s, cm, a) for r, s, _, _, cm, a, _ in R.SUM_ROWS_CASES])
def test_exact_sum_rows(dev, rows, stride, off, c, compact, accumulate, scale):
    """out[c] (+)= scale * sum_r partial[r * row_stride + col_offset + c] on integer rows: equality on both sides of the parallel
    and compaction thresholds, row_stride == 1 included; columns outside [col_offset, col_offset + C) do not enter."""
    k = Calls(dev, R.BF16)
    gen = torch.Generator().manual_seed(rows + stride)
    part = R.ints(gen, (rows * stride,), 50)
    out0 = R.ints(gen, (c,), 9)
    full = k.can.alloc(((rows + R.SCRATCH_ROWS) * stride,), torch.float32, "sum_rows partial")
    full[:rows * stride] = f32(part, dev)
    out = k.can.alloc((c,), torch.float32, "sum_rows out")
    out.copy_(f32(out0, dev))
    k.L.check(k.lib.dsr_pw_sum_rows(ptr(full), rows, stride, off, c, scale, ptr(out), accumulate, compact, stream()))
    k.can.check()
    same(out.cpu(), R.sum_rows(part, stride, off, c, scale, out0, accumulate), "sum_rows")


def test_bn_eval_affine(dev):
    """Eval-mode affine from the running statistics.  eps = 0 and variances that are powers of four: equality.  General values:
    rstd = 1 / sqrtf(var + eps) is three fp32 roundings, scale one more: 4 fp32 ulp; shift as in bn_finalize; pad channels 0."""
    k = Calls(dev, R.BF16)
    gen = torch.Generator().manual_seed(23)
    for cp in (8, 24, 136):
        c = R.C_OF_CP[cp]
        for exact in (True, False):
            if exact:
                gamma, beta, rm, eps = R.pow2(gen, (c,), -1, 1, signed=True), R.ints(gen, (c,), 3), R.ints(gen, (c,), 3), 0.0
                rv = R.pow2(gen, (c,), -1, 2) ** 2
            else:
                gamma, beta, rm = (torch.randn(c, generator=gen).double() for _ in range(3))          # fp32 values
                rv, eps = (0.1 + torch.rand(c, generator=gen)).double(), EPS
            outs = {q: k.can.alloc((cp,), torch.float32, "bn_eval_affine " + q) for q in ("scale", "shift", "mean", "rstd")}
            ins = [f32(v, dev) for v in (gamma, beta, rm, rv)]
            k.L.check(k.lib.dsr_pw_bn_eval_affine(*[ptr(v) for v in ins], eps, c, cp,
                                                  *[ptr(outs[q]) for q in ("scale", "shift", "mean", "rstd")], stream()))
            k.can.check()
            want = R.bn_eval_affine(gamma, beta, rm, rv, eps, c, cp)
            for q in outs:
                assert float(outs[q][c:].abs().sum()) == 0.0, q
                if exact or q == "mean":
                    same(outs[q].cpu(), want[q], q)
                elif q == "shift":
                    within(outs[q][:c], want[q][:c], 4 * U24 * (beta.abs() + (rm * want["scale"][:c]).abs()), q)
                else:
                    within(outs[q], want[q], 4 * R.ulp32(want[q]), q)


# ----------------------------------------------------------------------------- rounded regime
def real_on_device(d, q, dev, dtype):
    t = {key: up16(d[key], dtype, dev) for key in ("y", "dout", "residual", "dout_e2e")}
    t.update({key: f32(q[key], dev) for key in q})
    return t


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.REAL_IDS)
def test_rounded_outputs(dev, name, dtype):
    """bn_act_fwd (with residual) and act_bwd on real data, every activation (ELU, tanh and sigmoid run the run-time fallback
    of both kernels):
    each 16-bit result is one of the two storage-type neighbours of the float64 value computed from the same fp32 parameters;
    act_bwd's partial rows follow the summation-chain bound k * 2^-24 * sum |terms|."""
    k = Calls(dev, dtype)
    d = R.real_stream_cached(name, dtype)
    p, cp, c, rpb, rpi = (d["case"][q] for q in ("p", "cp", "c", "rpb", "rpi"))
    q = R.real_params(d, R.ACT_NONE, 0.0, rpb)
    t = real_on_device(d, q, dev, dtype)
    todo = []
    for act, slope in R.REAL_ACTS:
        tag = R.ACT_NAMES[act]
        # the residual takes the sign of the activation's output: a sum that cancels (|out + r| << |out|) carries the fp32 rounding
        # of `out`, which no evaluation in fp32 keeps inside an ulp of the tiny result; mixed signs are the exact regime's
        plain = R.bn_act_fwd(d["y"], q["scale"], q["shift"], None, act, slope)
        res64 = torch.where(plain < 0, -d["residual"].abs(), d["residual"].abs())
        amb = R.kink_ambiguous(d["y"], q["scale"], q["shift"], act)      # (a sign flip of a z next to zero changes its 16-bit image)
        got = k.bn_act_fwd(t["y"], t["scale"], t["shift"], up16(res64, dtype, dev), p, cp, act, slope)
        todo.append(("n", got, plain + res64, amb, "bn_act_fwd + residual " + tag))
        got = k.bn_act_fwd(t["y"], t["scale"], t["shift"], None, p, cp, act, slope)
        todo.append(("n", got, plain, amb, "bn_act_fwd " + tag))
        # act_bwd reads the stored 16-bit output (tanh / sigmoid / ELU through its run-time instantiation too: 1 - o^2 and
        # o (1 - o) of a 16-bit o are exact in fp32, so dy is one product away from the float64 value)
        o64 = R.r16(R.bn_act_fwd(d["y"], q["scale"], q["shift"], None, act, slope), dtype)
        dy, part, _ = k.act_bwd(t["dout"], up16(o64, dtype, dev), 1, 1, p, cp, cp, False, act, slope, rpb)
        wdy, wpart = R.act_bwd(d["dout"], o64, act, slope, rpb)
        aterm = (d["dout"] * (o64 / slope) * (o64 < 0)).abs() if act == R.ACT_PRELU else torch.zeros_like(wdy)
        apart = torch.stack([R.block_sums(wdy.abs(), rpb), R.block_sums(aterm, rpb)], 1)
        todo.append(("n", dy, wdy, None, "act_bwd dy " + tag))
        todo.append(("w", part, wpart, chain_k(rpb, rpi) * U24 * apart, "act_bwd partial " + tag))
    k.can.check()
    for kind, got, want, bound, what in todo:
        if kind == "n":
            neighbour(got, want, dtype, f"{name} {what}", allow=bound)
        else:
            within(got, want, bound, f"{name} {what}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.REAL_IDS)
def test_rounded_channel_stats_and_colsum(dev, name, dtype):
    """channel_stats on real data, large-mean channels included: per block |sum - ref| <= k * 2^-24 * sum |terms| with
    k = ceil(rpb / rpi) + rpi + 2 (a dropped or doubled row is an error of order 1 / rows_per_block of the sum: thousands of
    times this bound).  colsum likewise."""
    k = Calls(dev, dtype)
    d = R.real_stream_cached(name, dtype)
    p, cp, rpb, rpi = (d["case"][q] for q in ("p", "cp", "rpb", "rpi"))
    y = up16(d["y"], dtype, dev)
    _, got = k.channel_stats(y, p, cp, rpb)
    col = k.colsum(y, p, cp, rpb)
    k.can.check()
    kk = chain_k(rpb, rpi) * U24
    within(got, R.channel_stats(d["y"], rpb), kk * R.channel_stats(d["y"].abs(), rpb), name + " channel_stats")
    within(col, R.colsum(d["y"], rpb), kk * R.colsum(d["y"].abs(), rpb), name + " colsum")


def backward_bounds(d, q, dout, act, slope, rpb, rpi, p):
    """Reference rows and finalize results from the fp32 parameter arrays q, and their bounds.  Rows: k * 2^-24 * sum |terms| per
    block, plus, for the few elements whose pre-activation fp32 may put on the other side of the kink, the whole term.  dbeta
    (c1 = dbeta / count) inherits the row bound summed over the blocks; dgamma = rstd (sum g*y - mean sum g) (c2 likewise):
    rstd * k * 2^-24 * (sum |g*y| + |mean| sum |g|); each plus 4 fp32 ulp for the finalize kernel's own roundings."""
    c = d["case"]["c"]
    kk = chain_k(rpb, rpi) * U24
    ref = R.bn_act_bwd_reduce(dout, d["y"], q["scale"], q["shift"], act, slope, rpb)
    absr = R.bn_act_bwd_reduce_abs(dout, d["y"], q["scale"], q["shift"], act, slope, rpb)
    amb = R.kink_ambiguous(d["y"], q["scale"], q["shift"], act).double() * dout.abs()
    z = d["y"] * q["scale"] + q["shift"]
    extra = torch.stack([R.block_sums(amb, rpb), R.block_sums(amb * d["y"].abs(), rpb), R.block_sums(amb * z.abs(), rpb)], 1)
    row_bound = kk * absr + extra
    fin = R.bn_bwd_finalize(ref, c, d["case"]["cp"], float(p), q["mean"], q["rstd"])
    tot = row_bound.sum(0)
    b_dbeta = tot[0, :c]
    b_dgamma = q["rstd"][:c] * (tot[1, :c] + q["mean"][:c].abs() * tot[0, :c])
    bounds = dict(dbeta=b_dbeta + 4 * R.ulp32(fin["dbeta"]), dgamma=b_dgamma + 4 * R.ulp32(fin["dgamma"]),
                  c1=b_dbeta / p + 4 * R.ulp32(fin["c1"][:c]), c2=b_dgamma / p + 4 * R.ulp32(fin["c2"][:c]),
                  dprelu=tot[2, :c].sum() + 4 * R.ulp32(fin["dprelu"]))
    return ref, row_bound, fin, bounds


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.REAL_IDS)
def test_rounded_backward_reduce_and_finalize(dev, name, dtype):
    """bn_act_bwd_reduce -> bn_bwd_finalize on real data, every activation, large-mean channels included, against float64 from
    the same fp32 scale / shift / mean / rstd arrays (bounds: backward_bounds); pad channels of c1 / c2 exactly 0."""
    k = Calls(dev, dtype)
    d = R.real_stream_cached(name, dtype)
    p, cp, c, rpb, rpi = (d["case"][q] for q in ("p", "cp", "c", "rpb", "rpi"))
    q = R.real_params(d, R.ACT_NONE, 0.0, rpb)
    t = real_on_device(d, q, dev, dtype)
    blocks = R.n_blocks(p, rpb)
    todo = []
    for act, slope in R.REAL_ACTS:
        full, rows = k.bwd_reduce(t["dout"], t["y"], t["scale"], t["shift"], t["mean"], t["rstd"], p, cp, rpb, act, slope)
        fin = k.bn_bwd_finalize(full, blocks, c, cp, p, t["mean"], t["rstd"], act == R.ACT_PRELU)
        torch.cuda.synchronize()
        todo.append((act, slope, rows.cpu(), {key: (None if v is None else v.cpu()) for key, v in fin.items()}))
    k.can.check()
    for act, slope, rows, fin in todo:
        tag = f"{name} {R.ACT_NAMES[act]} "
        ref, row_bound, want, bounds = backward_bounds(d, q, d["dout"], act, slope, rpb, rpi, p)
        within(rows, ref, row_bound, tag + "rows")
        for key in ("dgamma", "dbeta"):
            within(fin[key], want[key], bounds[key], tag + key)
        for key in ("c1", "c2"):
            within(fin[key][:c], want[key][:c], bounds[key], tag + key)
            assert float(fin[key][c:].abs().sum()) == 0.0, tag + key + " pad channels"
        if act == R.ACT_PRELU:
            within(fin["dprelu"], want["dprelu"].reshape(1), bounds["dprelu"].reshape(1), tag + "dprelu")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.REAL_IDS)
def test_rounded_backward_apply(dev, name, dtype):
    """bn_act_bwd_apply in train mode against float64 from the same fp32 parameter arrays.  The kernel forms dy = A g + B y + C
    with A = scale, B = -scale c2 rstd, C = scale (c2 mean rstd - c1) in fp32.  Counting roundings (units of 2^-24 relative):
    A g: g 1, the product 1, the two additions 2; B y: B 2, product 1, additions 2; C: 4, additions up to 2 -- at most 6 on any
    term, inside the constant 8 the bound is stated with.  For ELU / tanh / sigmoid g = dout * act'(z) costs more and the
    count replaces the 8: act' from exp(-|z|) takes 8 (exponential 2, sum 1, reciprocal and product 3, two products 2), and the one
    rounding of z = fma(y, scale, shift) enters act' with the sensitivity |d log act' / dz| |z| <= 2 |z|, so A g carries
    8 + 2 max|z| + 4 (max|z| from the reference's own pre-activations).  Plus one storage ulp of the result for the final
    rounding to 16 bits.  Eval mode (dy = scale g): a neighbour of the float64 value; for ELU / tanh / sigmoid the same count on
    its one term."""
    k = Calls(dev, dtype)
    d = R.real_stream_cached(name, dtype)
    p, cp, c, rpb = (d["case"][q] for q in ("p", "cp", "c", "rpb"))
    todo = []
    for act, slope in R.REAL_ACTS:
        q = R.real_params(d, act, slope, rpb)
        t = real_on_device(d, q, dev, dtype)
        args = (t["dout"], t["y"], t["scale"], t["shift"], t["mean"], t["rstd"], t["c1"], t["c2"], p, cp, act, slope)
        todo.append((act, slope, q, k.bwd_apply(*args, True), k.bwd_apply(*args, False)))
    k.can.check()
    for act, slope, q, train, evalm in todo:
        tag = f"{name} {R.ACT_NAMES[act]} "
        ref_args = (d["dout"], d["y"], q["scale"], q["shift"], q["mean"], q["rstd"], q["c1"], q["c2"], act, slope)
        amb = R.kink_ambiguous(d["y"], q["scale"], q["shift"], act)
        ref = R.bn_act_bwd_apply(*ref_args, True)
        zmax = float((d["y"] * q["scale"] + q["shift"]).abs().max())
        count = 8 if act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY, R.ACT_PRELU) else 12 + 2 * zmax
        within(train, ref, count * U24 * R.bn_act_bwd_apply_terms(*ref_args) + R.ulp16(ref, dtype), tag + "train", allow=amb)
        ref_eval = R.bn_act_bwd_apply(*ref_args, False)
        if act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY, R.ACT_PRELU):
            neighbour(evalm, ref_eval, dtype, tag + "eval", allow=amb)
        else:      # dy = scale * g with the counted roundings of g, and the rounding to 16 bits
            within(evalm, ref_eval, count * U24 * ref_eval.abs() + R.ulp16(ref_eval, dtype), tag + "eval")
        assert float(train[:, c:].float().abs().sum()) == 0.0 and float(evalm[:, c:].float().abs().sum()) == 0.0, tag + "pad channels"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", R.E2E_IDS)
def test_end_to_end_train_step(dev, name, dtype):
    """The three-launch forward (channel_stats -> bn_finalize -> bn_act_fwd) and the three-launch backward (bn_act_bwd_reduce ->
    bn_bwd_finalize -> bn_act_bwd_apply) wired as the product wires them (count = P, grids from dsr_pw_reduce_blocks), against
    the float64 reference on the rounded input, large-mean channels included.  dx within 2 storage ulp of the reference
    wherever |ref| exceeds 2^-6 of its channel's largest |ref|, within 2^-7 of that largest value elsewhere (under 5 % of the
    elements: test_host_pointwise.py); dgamma / dbeta within the summation-chain bounds; pad channels zero."""
    k = Calls(dev, dtype)
    d = R.real_stream_cached(name, dtype)
    p, cp, c, rpi = (d["case"][q] for q in ("p", "cp", "c", "rpi"))
    rpb = C.c_int(0)
    blocks = k.lib.dsr_pw_reduce_blocks(p, C.byref(rpb))
    rpb = rpb.value
    y, dout = up16(d["y"], dtype, dev), up16(d["dout_e2e"], dtype, dev)
    gamma, beta = f32(d["gamma"], dev), f32(d["beta"], dev)
    results = []
    for act, slope in R.REAL_ACTS:
        full, _ = k.channel_stats(y, p, cp, rpb)
        fin = k.bn_finalize(full, blocks, cp, c, cp, p, gamma, beta, None, None, None, 0)
        out = k.bn_act_fwd(y, fin["scale"], fin["shift"], None, p, cp, act, slope)
        full, _ = k.bwd_reduce(dout, y, fin["scale"], fin["shift"], fin["mean"], fin["rstd"], p, cp, rpb, act, slope)
        bw = k.bn_bwd_finalize(full, blocks, c, cp, p, fin["mean"], fin["rstd"], act == R.ACT_PRELU)
        dx = k.bwd_apply(dout, y, fin["scale"], fin["shift"], fin["mean"], fin["rstd"], bw["c1"], bw["c2"], p, cp, act, slope, True)
        torch.cuda.synchronize()
        results.append((act, slope, out.cpu(), dx.cpu(), bw["dgamma"].cpu(), bw["dbeta"].cpu()))
    k.can.check()
    for act, slope, out, dx, dgamma, dbeta in results:
        tag = f"{name} {R.ACT_NAMES[act]} "
        ref = R.bn_train_act(d["y"], c, d["gamma"], d["beta"], EPS, act, slope, d["dout_e2e"], rpb=rpb)
        q = {key: ref["fin"][key] for key in ("scale", "shift", "mean", "rstd")}
        amb = R.kink_ambiguous(d["y"], q["scale"], q["shift"], act)
        top = ref["dx"].abs().amax(0, keepdim=True)
        rel = ref["dx"].abs() > 2.0 ** -6 * top
        assert float((~rel[:, :c]).double().mean()) <= 0.05
        bound = torch.where(rel, 2 * R.ulp16(ref["dx"], dtype), 2.0 ** -7 * top + torch.zeros_like(ref["dx"]))
        within(dx, ref["dx"], bound, tag + "dx", allow=amb)
        assert float(dx[:, c:].float().abs().sum()) == 0.0 and (act == R.ACT_SIGMOID or float(out[:, c:].float().abs().sum()) == 0.0)
        _, _, want, bounds = backward_bounds(d, q, d["dout_e2e"], act, slope, rpb, rpi, p)
        within(dgamma, want["dgamma"], bounds["dgamma"], tag + "dgamma")
        within(dbeta, want["dbeta"], bounds["dbeta"], tag + "dbeta")
