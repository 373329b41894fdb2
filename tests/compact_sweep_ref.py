"""Case tables, operands, float64 yardsticks, the slope-gradient band and an fp32 emulation for the sweep of the compact pointwise
kernels (csrc/pw_compact.hip) past their first regime: tests/test_gpu_compact_sweep.py launches the kernels against these through
the raw C ABI, and tests/test_host_compact_sweep.py shows on the CPU that every case is in the regime it claims, that the emulation
in the kernel's own order is inside the band and that the listed wrong variants are outside it (or unequal on the exact data).
The formulas themselves are tests/compact_ref.py's (prelu_c, prelu_bwd, shuffle_add, shuffle_add_bwd, small_ints, exact_slopes);
nothing is restated here but the LAUNCH GEOMETRY, which is what the sweep is about:

  dsr_pw_prelu_c_bwd   rows = min(1024, ceil(P / 64)) blocks, ppr = ceil(P / rows) pixels per block; a block of 256 threads is
                       npl = 256 // (Cp / 8) pixel lanes of Cp / 8 chunk threads (256 - npl * Cp / 8 threads idle); lane l takes
                       pixels p0 + l, p0 + l + npl, ... in order, row r of `partial` is the sum over the lanes in lane order; the
                       fold gives thread t of 64 the rows t, t + 64, ... in order, then an xor butterfly (32, 16, .., 1).
  pc_grid              every elementwise launch is capped at 8192 blocks of 256 threads and strides over the rest.

The band of the slope gradient (u = 2^-24, the products dy * z of two 16-bit values are exact in fp32):
    |dslope_c - sum_f64| <= depth * u * sum over the pixels with z <= 0 of |dy z|,
    depth = ceil(ppr / npl) + npl + ceil(rows / 64) + 6
(the terms a thread adds, the adds over the block's lanes, the adds of a fold thread, the six butterfly steps).  The sum of
magnitudes runs over the terms that are added, not over every pixel: the narrower of the two readings."""
import functools

import numpy as np
import torch

import compact_ref as R

FOLD_W = 64                   # dsr_pw_prelu_c_fold_width()
MIN_PIX = 64                  # pixels per partial row, at least
MAX_ROWS = 1024               # the cap on partial rows
GRID_THREADS = 8192 * 256     # pc_grid: threads of one grid pass
ELEM_LIMIT = 0x7FFFFFFF       # the shuffle entry points refuse this many elements or more
U = 2.0 ** -24

# ----------------------------------------------------------------------------- case tables
BWD_PIXELS = [65536, 65537, 3 * 65536 + 5]                 # Cp = C = 64: on the cap; empty trailing rows; several pixels a lane
FLOAT_PIXELS = [65537, 3 * 65536 + 5]
LAYOUTS = [(8, 8), (20, 24), (70, 72), (2048, 2048)]       # (C, Cp)
WIDE = (2048, 2048)                                        # one pixel lane: small pixel counts only
WIDE_PIXELS = [130, 4161]
FWD_CAP_CASES = [(64, 64, 262144 + 37), (20, 24, 699051 + 37)]          # (C, Cp, P): P * Cp / 8 > 8192 * 256

SHUFFLE_SMALL = [(2, 3, 37, 41), (1, 5, 9, 130)]           # (N, C, H, W) of the LR side, every s in 1..4: past one block
SHUFFLE_FWD_LARGE = [(4, (2, 3, 150, 150)), (1, (2, 3, 600, 592))]      # (s, shape): output elements past one grid pass
SHUFFLE_BWD_LARGE = [(1, (2, 3, 600, 592)), (2, (2, 3, 600, 592))]      # LR pixels past one grid pass
SHUFFLE_NULL_SMALL = (3, (2, 3, 37, 41))                   # base == NULL / dbase == NULL at a small shape
SHUFFLE_NULL_FWD_LARGE = SHUFFLE_FWD_LARGE[0]
SHUFFLE_NULL_BWD_LARGE = SHUFFLE_BWD_LARGE[0]


def rows_of(p):
    """dsr_pw_prelu_c_rows restated (the host test holds this against the built library)."""
    return min(MAX_ROWS, -(-p // MIN_PIX)) if p > 0 else 0


def geometry(p, cp, rows=None):
    """dict(rows, ppr, used, empty, last, chunks, npl, idle, per_thread, fold_turns, fold_adds, depth) of one backward launch.
    used: rows that own a pixel, empty: rows that own none, last: pixels of the last used row.  rows: from the library's
    query when given."""
    rows = rows_of(p) if rows is None else rows
    ppr = -(-p // rows)
    used = -(-p // ppr)
    chunks = cp // 8
    npl = 256 // chunks
    per_thread = -(-ppr // npl)
    fold_adds = -(-rows // FOLD_W)
    return dict(rows=rows, ppr=ppr, used=used, empty=rows - used, last=p - (used - 1) * ppr, chunks=chunks, npl=npl,
                idle=256 - npl * chunks, per_thread=per_thread, fold_turns=-(-cp // 256), fold_adds=fold_adds,
                depth=per_thread + npl + fold_adds + 6)


def layout_pixels(c, cp):
    """The pixel counts a layout is run at: fold_width * ppr + 1 as tests/test_gpu_compact.py takes it from the query (ppr = 64
    while there are fewer than 1024 rows), and 65 537; the 2048-channel layout at 130 and 4161 only."""
    return list(WIDE_PIXELS) if (c, cp) == WIDE else [FOLD_W * MIN_PIX + 1, 65537]


def bwd_cases():
    """[(C, Cp, P)] of the exact backward sweep, each once."""
    out = [(64, 64, p) for p in BWD_PIXELS]
    for c, cp in LAYOUTS:
        out += [(c, cp, p) for p in layout_pixels(c, cp)]
    return out


def grid_threads(n):
    """(threads launched, elements the first thread takes) of an elementwise launch over n elements."""
    threads = min(GRID_THREADS, -(-n // 256) * 256)
    return threads, -(-n // threads)


# ----------------------------------------------------------------------------- operands and yardsticks: pointwise PReLU
def nchw(t):
    """[P, C] -> the [1, C, 1, P] view compact_ref's formulas take."""
    return t.t().reshape(1, t.shape[1], 1, t.shape[0])


def flat(t4):
    """[1, C, 1, P] -> [P, C]."""
    return t4.reshape(t4.shape[1], t4.shape[3]).t().contiguous()


@functools.lru_cache(maxsize=2)
def exact_case(c, p):
    """Integer operands [P, C] and their float64 yardsticks, as a dict of read-only tensors: z in [-6, 6] with zeros, dy in
    [-3, 3], slopes from {0, +-2^k} differing per channel.  y, dz: [P, C]; dslope: [C].  Everything is exact in bf16, fp16 and
    fp32, and sum |dy z| <= 18 P < 2^24 (asserted)."""
    g = torch.Generator().manual_seed(100003 * c + p)
    z, dy = R.small_ints(g, (p, c), 6), R.small_ints(g, (p, c), 3)
    slope = R.exact_slopes(c)
    assert 18 * p < 2 ** 24 and bool((z == 0).any())
    dz, dslope = R.prelu_bwd(nchw(dy), nchw(z), slope)
    return dict(z=z, dy=dy, slope=slope, y=flat(R.prelu_c(nchw(z), slope)), dz=flat(dz), dslope=dslope)


@functools.lru_cache(maxsize=1)
def exact_fwd_case(c, p):
    """The forward alone (the large cases past the grid cap): z [P, C] in [-6, 6], slopes, y = prelu_c(z)."""
    g = torch.Generator().manual_seed(100019 * c + p)
    z = R.small_ints(g, (p, c), 6)
    slope = R.exact_slopes(c)
    return dict(z=z, slope=slope, y=flat(R.prelu_c(nchw(z), slope)))


@functools.lru_cache(maxsize=2)
def float_case(dtype, p, c=64):
    """N(0, 1) z and dy stored in the 16-bit type, slopes in [-1.5, 1.5] (fp32 values; channel 5 zero): the float64 dslope [C]
    and the sum of |dy z| over the pixels with z <= 0, per channel."""
    g = torch.Generator().manual_seed(31 * p + dtype)
    t16 = lambda t: t.to(R.DTYPES[dtype]).double()
    z = t16(torch.randn(p, c, generator=g, dtype=torch.float64))
    dy = t16(torch.randn(p, c, generator=g, dtype=torch.float64))
    slope = (torch.rand(c, generator=g, dtype=torch.float64) * 3.0 - 1.5).float().double()
    slope[5] = 0.0
    dz, dslope = R.prelu_bwd(nchw(dy), nchw(z), slope)
    mag = ((dy * z).abs() * (z <= 0)).sum(dim=0)
    return dict(z=z, dy=dy, slope=slope, dz=flat(dz), dslope=dslope, mag=mag)


def band(p, cp, mag, rows=None):
    """float64 [C]: depth * 2^-24 * sum |dy z| (module docstring)."""
    return geometry(p, cp, rows)["depth"] * U * mag


def worst_ratio(got, want, bound):
    err = (got.double() - want).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def row_sums(case, p, cp):
    """float64 [rows, C]: the exact value of every partial row (empty rows zero)."""
    geo = geometry(p, cp)
    z, dy = case["z"], case["dy"]
    c = z.shape[1]
    terms = torch.zeros(geo["rows"] * geo["ppr"], c, dtype=torch.float64)
    terms[:p] = dy * z * (z <= 0)
    return terms.view(geo["rows"], geo["ppr"], c).sum(dim=1)


def emulate_dslope(case, p, cp, drop_last_row=False, double_row=None):
    """float32 [C]: the slope gradient in the kernel's own order, one fp32 rounding per add.  drop_last_row: the WRONG variant
    whose fold stops one short of the last row that owns a pixel; double_row: the WRONG variant that adds that row twice."""
    geo = geometry(p, cp)
    rows, ppr, npl, k = geo["rows"], geo["ppr"], geo["npl"], geo["per_thread"]
    z, dy = case["z"].numpy(), case["dy"].numpy()
    c = z.shape[1]
    terms = np.zeros((rows * ppr, c), dtype=np.float32)
    prod = (dy * z * (z <= 0)).astype(np.float32)
    assert np.array_equal(prod.astype(np.float64), dy * z * (z <= 0)), "a product of two 16-bit values is exact in fp32"
    terms[:p] = prod
    padded = np.zeros((rows, k * npl, c), dtype=np.float32)            # pixel q of a row: turn q // npl of lane q % npl
    padded[:, :ppr] = terms.reshape(rows, ppr, c)
    v = padded.reshape(rows, k, npl, c)
    acc = np.zeros((rows, npl, c), dtype=np.float32)
    for t in range(k):
        acc = acc + v[:, t]
    part = np.zeros((rows, c), dtype=np.float32)
    for l in range(npl):
        part = part + acc[:, l]
    if drop_last_row:
        part[geo["used"] - 1] = 0
    if double_row is not None:
        part[double_row] = part[double_row] * np.float32(2)
    turns = geo["fold_adds"]
    tab = np.zeros((turns * FOLD_W, c), dtype=np.float32)
    tab[:rows] = part
    tab = tab.reshape(turns, FOLD_W, c)
    s = np.zeros((FOLD_W, c), dtype=np.float32)
    for t in range(turns):
        s = s + tab[t]
    lane = np.arange(FOLD_W)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ o]
    assert s.dtype == np.float32
    return torch.from_numpy(s[0].copy())


# ----------------------------------------------------------------------------- operands and yardsticks: shuffle-add
@functools.lru_cache(maxsize=2)
def shuffle_case(s, shape):
    """Integer operands in [-50, 50] and the float64 yardsticks of both directions, read only: t [N, C s^2, H, W], base
    [N, C, H, W], dout [N, C, sH, sW]; out / out_nobase [N, C, sH, sW]; dt, dbase."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(7 * s + n + 3 * c + 5 * h + 11 * w)
    t, base = R.small_ints(g, (n, c * s * s, h, w), 50), R.small_ints(g, (n, c, h, w), 50)
    dout = R.small_ints(g, (n, c, s * h, s * w), 50)
    dt, dbase = R.shuffle_add_bwd(dout, s)
    return dict(t=t, base=base, dout=dout, out=R.shuffle_add(t, base, s), out_nobase=R.shuffle_add(t, None, s), dt=dt, dbase=dbase)


def clear():
    for f in (exact_case, exact_fwd_case, float_case, shuffle_case):
        f.cache_clear()
