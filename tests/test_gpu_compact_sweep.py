"""GPU: the compact pointwise kernels (csrc/pw_compact.hip) past their first regime, through the raw C ABI, against float64 (case
tables, yardsticks, the band and its derivation: tests/compact_sweep_ref.py; the regimes, the fp32 emulation inside the band and
the wrong variants outside it, on the CPU: tests/test_host_compact_sweep.py).  tests/test_gpu_compact.py stops at 65 partial rows
of 64 pixels, Cp = 64 and 16, one grid pass and 2 x 3 x 5 x 7 shuffles; here

  dsr_pw_prelu_c_bwd    on the cap of 1024 partial rows, one pixel past it (ppr = 65, fifteen empty rows that must still be
                        written) and three times past it; chunk counts that leave idle threads (Cp = 24, 72), 256 pixel lanes
                        (Cp = 8) and one pixel lane with eight turns of the per-block fold (Cp = 2048); partial == dslope == NULL
  dsr_pw_prelu_c_fwd    the same layouts, and a second grid-stride turn
  dsr_shuffle_add_f32 / _bwd_f32   past one block at every s, a second grid-stride turn, base == NULL and dbase == NULL

Every raw output sits between sentinel margins and is pre-filled with NaN; inputs sit between NaN margins, so a read past an end
(a slope of a pad channel, say) shows in the result."""
import ctypes as C
import importlib
import math

import pytest
import torch

import compact_ref as R
import compact_sweep_ref as S

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
NAN = float("nan")
MARGIN = 1024
DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    yield torch.device("cuda:0")
    S.clear()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Raw:
    """Device buffers between MARGIN sentinel elements on each side; check() asserts that every margin kept its bits."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, shape, dtype, fill=NAN, margin=7777.0):
        numel = math.prod(shape)
        flat = torch.full((numel + 2 * MARGIN,), margin, dtype=dtype, device=self.dev)
        flat[MARGIN:MARGIN + numel] = fill
        self.bufs.append((flat, _bits(flat[:MARGIN]).clone(), _bits(flat[-MARGIN:]).clone()))
        return flat[MARGIN:MARGIN + numel].view(shape)

    def put(self, t):
        v = self.new(tuple(t.shape), t.dtype, 0, NAN)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, lo, hi in self.bufs:
            assert torch.equal(_bits(flat[:MARGIN]), lo) and torch.equal(_bits(flat[-MARGIN:]), hi), "write outside a buffer"


def _padded(t, cp, dtype, exact=True):
    """float64 [P, C] -> the 16-bit [P, Cp] tensor the kernels take, pad channels zero."""
    p, c = t.shape
    out = torch.zeros(p, cp, dtype=R.DTYPES[dtype])
    out[:, :c] = t.to(R.DTYPES[dtype])
    if exact:
        assert torch.equal(out[:, :c].double(), t), "operand not representable"
    return out


def _fwd(dev, dtype, z, slope, cp, exact=True):
    """One dsr_pw_prelu_c_fwd launch: y [P, Cp] on the host, as stored."""
    L = P("_lib")
    p, c = z.shape
    raw = Raw(dev)
    zd, sd = raw.put(_padded(z, cp, dtype, exact)), raw.put(slope.float())
    yd = raw.new((p, cp), R.DTYPES[dtype])
    L.check(L.lib().dsr_pw_prelu_c_fwd(dtype, _ptr(zd), _ptr(sd), _ptr(yd), p, c, cp, _st()))
    raw.check()
    return yd.cpu()


def _bwd(dev, dtype, case, cp, with_partial=True, exact=True):
    """One dsr_pw_prelu_c_bwd call: (dz [P, Cp], partial [rows, Cp] or None, dslope [C] or None) on the host, as stored."""
    L = P("_lib")
    lib = L.lib()
    p, c = case["z"].shape
    rows = lib.dsr_pw_prelu_c_rows(p)
    raw = Raw(dev)
    zd, gd = raw.put(_padded(case["z"], cp, dtype, exact)), raw.put(_padded(case["dy"], cp, dtype, exact))
    sd = raw.put(case["slope"].float())
    dz = raw.new((p, cp), R.DTYPES[dtype])
    part = raw.new((rows, cp), torch.float32) if with_partial else None
    dslope = raw.new((c,), torch.float32) if with_partial else None
    L.check(lib.dsr_pw_prelu_c_bwd(dtype, _ptr(gd), _ptr(zd), _ptr(sd), _ptr(dz), p, c, cp, _ptr(part), _ptr(dslope), _st()))
    raw.check()
    return dz.cpu(), None if part is None else part.cpu(), None if dslope is None else dslope.cpu()


# ============================================================================= 1. the pointwise PReLU on integers
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c,cp,p", S.bwd_cases(), ids=lambda v: str(v))
def test_prelu_exact_past_the_row_cap_and_in_every_layout(dev, dtype, c, cp, p):
    """Integers in [-6, 6] with zeros, dy in [-3, 3], slopes from {0, +-2^k}: y, dz, EVERY row of `partial` (the empty ones are
    zero, none keeps its NaN) and dslope compared with ==; pad channels of y, dz and partial zero; dslope has C entries and the
    sentinel behind them is intact."""
    lib = P("_lib").lib()
    case = S.exact_case(c, p)
    geo = S.geometry(p, cp, lib.dsr_pw_prelu_c_rows(p))
    y = _fwd(dev, dtype, case["z"], case["slope"], cp)
    assert torch.equal(y[:, :c].double(), case["y"]) and not bool(y[:, c:].any()) and not bool(torch.isnan(y.float()).any())
    dz, part, dslope = _bwd(dev, dtype, case, cp)
    assert torch.equal(dz[:, :c].double(), case["dz"]), float((dz[:, :c].double() - case["dz"]).abs().max())
    assert not bool(torch.isnan(dz.float()).any()) and not bool(dz[:, c:].any())
    assert tuple(part.shape) == (geo["rows"], cp) and not bool(torch.isnan(part).any()), "a partial row was not written"
    want_rows = S.row_sums(case, p, cp)
    assert torch.equal(part[:, :c].double(), want_rows) and not bool(part[:, c:].any())
    assert not bool(part[geo["used"]:].any())
    assert tuple(dslope.shape) == (c,) and torch.equal(dslope.double(), case["dslope"]), float((dslope.double() - case["dslope"]).abs().max())


@pytest.mark.parametrize("dtype", DT)
def test_prelu_bwd_without_a_slope_gradient(dev, dtype):
    """partial == dslope == NULL one pixel past the row cap: dz has the bits of the call that also forms the slope gradient, and
    the launch log holds the one entry-point call (the fold of a NULL table would be a fault, not a wrong number)."""
    L = P("_lib")
    p = 65537
    case = S.exact_case(64, p)
    full, _, _ = _bwd(dev, dtype, case, 64)
    L.LAUNCH_LOG = log = []
    try:
        alone, part, dslope = _bwd(dev, dtype, case, 64, with_partial=False)
    finally:
        L.LAUNCH_LOG = None
    assert part is None and dslope is None
    assert [name for name, _, _ in log] == ["dsr_pw_prelu_c_bwd"]
    assert torch.equal(_bits(alone), _bits(full)) and torch.equal(alone.double(), case["dz"])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c,cp,p", S.FWD_CAP_CASES, ids=lambda v: str(v))
def test_prelu_fwd_takes_a_second_grid_turn(dev, dtype, c, cp, p):
    """P * Cp / 8 vectors on 8192 * 256 threads: the first threads take a second vector.  == on integers, pad channels zero."""
    assert p * cp // 8 > S.GRID_THREADS
    case = S.exact_fwd_case(c, p)
    y = _fwd(dev, dtype, case["z"], case["slope"], cp)
    assert not bool(torch.isnan(y.float()).any())
    assert torch.equal(y[:, :c].double(), case["y"]) and not bool(y[:, c:].any())


# ============================================================================= 2. the slope gradient on float data
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("p", S.FLOAT_PIXELS)
def test_dslope_float_within_the_band_and_equal_bits(dev, dtype, p):
    """N(0, 1) z and dy in the 16-bit type: |dslope - f64| <= depth 2^-24 sum |dy z| per channel, depth = ceil(ppr / npl) + npl +
    ceil(rows / 64) + 6 = 57 at P = 65 537 and 61 at P = 196 613 (tests/compact_sweep_ref.py); dz the product rounded to 16 bits;
    two runs give equal bits.  A dropped or doubled partial row and a mask taken from the output are outside this band
    (tests/test_host_compact_sweep.py).
    Observed on the MI355X, worst |hip - f64| / band: P = 65 537 bf16 0.00076, fp16 0.00105; P = 196 613 bf16 0.00042, fp16
    0.00049 -- each the figure of the CPU emulation of the kernel's order to the digits it prints.  The band is a worst case over
    57 or 61 roundings of sums that in fact grow like a random walk, hence the distance.  These are measurements; the band is the
    derived one."""
    lib = P("_lib").lib()
    case = S.float_case(dtype, p)
    bound = S.band(p, 64, case["mag"], lib.dsr_pw_prelu_c_rows(p))
    runs = [_bwd(dev, dtype, case, 64, exact=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    dz, part, dslope = runs[0]
    assert not bool(torch.isnan(part).any()) and not bool(torch.isnan(dslope).any())
    # dz is the product dy * slope rounded to 16 bits, directly or through fp32: never farther from it than the storage model
    want = case["dz"]
    assert bool(((dz.double() - want).abs() <= (R._store(want, dtype) - want).abs()).all())
    ratio = S.worst_ratio(dslope, case["dslope"], bound)
    print(f"dslope float {dtype} P={p}: worst |hip - f64| / band = {ratio:.5f}")
    assert ratio <= 1.0


# ============================================================================= 3. shuffle-add, both directions
def _shuffle_fwd(dev, case, s, shape, with_base=True):
    L = P("_lib")
    n, c, h, w = shape
    raw = Raw(dev)
    td = raw.put(case["t"].float())
    bd = raw.put(case["base"].float()) if with_base else None
    out = raw.new((n, c, s * h, s * w), torch.float32)
    L.check(L.lib().dsr_shuffle_add_f32(_ptr(td), _ptr(bd), _ptr(out), n, c, s, h, w, _st()))
    raw.check()
    assert torch.equal(td.cpu().double(), case["t"])
    return out.cpu()


def _shuffle_bwd(dev, case, s, shape, with_dbase=True):
    L = P("_lib")
    n, c, h, w = shape
    raw = Raw(dev)
    gd = raw.put(case["dout"].float())
    dt = raw.new((n, c * s * s, h, w), torch.float32)
    dbase = raw.new((n, c, h, w), torch.float32) if with_dbase else None
    L.check(L.lib().dsr_shuffle_add_bwd_f32(_ptr(gd), _ptr(dt), _ptr(dbase), n, c, s, h, w, _st()))
    raw.check()
    return dt.cpu(), None if dbase is None else dbase.cpu()


def _check_fwd(dev, s, shape, with_base=True):
    case = S.shuffle_case(s, tuple(shape))
    out = _shuffle_fwd(dev, case, s, shape, with_base)
    want = case["out"] if with_base else case["out_nobase"]
    assert not bool(torch.isnan(out).any()), "an output element was not written"
    assert torch.equal(out.double(), want), float((out.double() - want).abs().max())


def _check_bwd(dev, s, shape, with_dbase=True):
    case = S.shuffle_case(s, tuple(shape))
    dt, dbase = _shuffle_bwd(dev, case, s, shape, with_dbase)
    assert not bool(torch.isnan(dt).any()) and torch.equal(dt.double(), case["dt"])
    assert (dbase is None) == (not with_dbase)
    if with_dbase:
        assert not bool(torch.isnan(dbase).any()) and torch.equal(dbase.double(), case["dbase"])


@pytest.mark.parametrize("shape", S.SHUFFLE_SMALL, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_shuffle_add_pair_past_one_block(dev, s, shape):
    _check_fwd(dev, s, shape)
    _check_bwd(dev, s, shape)


@pytest.mark.parametrize("s,shape", S.SHUFFLE_FWD_LARGE, ids=lambda v: str(v))
def test_shuffle_add_takes_a_second_grid_turn(dev, s, shape):
    assert math.prod(shape) * s * s > S.GRID_THREADS
    _check_fwd(dev, s, shape)


@pytest.mark.parametrize("s,shape", S.SHUFFLE_BWD_LARGE, ids=lambda v: str(v))
def test_shuffle_add_bwd_takes_a_second_grid_turn(dev, s, shape):
    assert math.prod(shape) > S.GRID_THREADS
    _check_bwd(dev, s, shape)


@pytest.mark.parametrize("s,shape", [S.SHUFFLE_NULL_SMALL, S.SHUFFLE_NULL_FWD_LARGE], ids=lambda v: str(v))
def test_shuffle_add_without_a_base(dev, s, shape):
    """base == NULL: the pixel shuffle alone (functional.ShuffleAdd never passes it)."""
    _check_fwd(dev, s, shape, with_base=False)


@pytest.mark.parametrize("s,shape", [S.SHUFFLE_NULL_SMALL, S.SHUFFLE_NULL_BWD_LARGE], ids=lambda v: str(v))
def test_shuffle_add_bwd_without_a_base_gradient(dev, s, shape):
    _check_bwd(dev, s, shape, with_dbase=False)
