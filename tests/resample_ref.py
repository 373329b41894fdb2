"""Float64 reference of the resampling / data-movement kernels of csrc/resample.hip, and the case tables of their sweep.

Every entry point is restated at index level from its contract (include/dsr_hip.h and the kernel comments) as plain float64
torch on NHWC [N, H, W, C] data (fp32 NCHW for resize_norm's image and for the downsampler), without calling the torch op it
restates: tests/test_host_resample.py pins each restatement against that op in float64.  Nothing is imported from the package
under test.  Where a bound needs it, a function also returns A, the sum of the absolute values of the terms of each result.

Conventions the reference follows:
  max pool     floor mode; scan order (0,0),(0,1),(1,0),(1,1); the running maximum is replaced when v > m or v is NaN, so a NaN
               propagates, the last NaN of a window owns it and among other values the first maximum does.  The backward routes
               dy to that element; every other element, and a trailing odd row / column, gets 0.  The ReLU-masked backward is
               the same with 0 where the window's maximum is <= 0; it is defined for finite non-negative x and +Inf only.
  avg pool     floor mode, (a + b + c + d) / 4; the adjoint hands dy / 4 to the four elements, 0 to a trailing row / column
  nearest x2   y[oy][ox] = x[oy // 2][ox // 2]; the adjoint sums each 2x2 block of dy
  bilinear x2  align_corners=False: source coordinate s = max(0, (o + 0.5) / 2 - 0.5), i0 = floor(s), i1 = min(i0 + 1, n - 1),
               weights 1 - (s - i0) and s - i0; the adjoint scatters the same weights
  resize_norm  out[n][oy][ox][c] = (sum_ij wy[oy][i] wx[ox][j] src[n][c][ys[oy] + i][xs[ox] + j] - mean[c]) / std[c] from the
               packed tables (start[o], count[o], w[o * KT + i]) exactly as given (fp32 values widened); channels C..7 are 0.
               The backward reads the TRANSPOSED tables (per input index: first output, count, weights).
  downsampler  y = strided correlation of the replicate-padded x with a k x k kernel; the adjoint scatters through the clamp

Two data regimes.  Exact: values on integer grids chosen so that every reference result is representable in bf16 and in fp16
(test_host_resample.py checks this), compared with equality; copies on arbitrary 16-bit patterns, compared as int16.  Rounded:
N(0,1) data against  |got - ref| <= u16 (|ref| + delta) + delta + floor,  delta = k 2^-24 A  (bound16), where k counts the
fp32 roundings of the kernel's chain and is stated at each check in tests/test_gpu_resample.py; fp32 outputs use delta alone."""
import functools

import numpy as np
import torch

BF16, F16 = 0, 1
DTYPES = {BF16: torch.bfloat16, F16: torch.float16}
U16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}          # unit roundoff of the storage types (8 and 11 significant bits)
FLOOR16 = {BF16: 0.0, F16: 2.0 ** -25}            # half of fp16's smallest subnormal; bf16 has fp32's range
U24 = 2.0 ** -24                                  # one fp32 rounding, relative
INF, NAN = float("inf"), float("nan")
F16_MAX = 65504.0


def r8(c):
    return (c + 7) // 8 * 8


def r16(t, dtype):
    """float64 -> fp32 -> the 16-bit storage type (round to nearest even) -> float64."""
    return t.to(torch.float32).to(DTYPES[dtype]).to(torch.float64)


def representable(t, dtype):
    return bool(torch.equal(r16(t, dtype), t.to(torch.float64)))


def bound16(ref, a, k, dtype):
    """|got - ref| for a 16-bit result of an fp32 chain of k roundings whose terms sum to A in absolute value."""
    delta = k * U24 * a
    return U16[dtype] * (ref.abs() + delta) + delta + FLOOR16[dtype]


def bound32(a, k):
    return k * U24 * a


# ----------------------------------------------------------------------------- 2x2 pools
SCAN = ((0, 0), (0, 1), (1, 0), (1, 1))


def _windows(x):
    """The four elements of every 2x2 window, in scan order: 4 x [N, H // 2, W // 2, C]."""
    oh, ow = x.shape[1] // 2, x.shape[2] // 2
    return [x[:, i:2 * oh:2, j:2 * ow:2] for i, j in SCAN]


def maxpool2_scan(x):
    """(maximum, index 0..3 of the element the scan ends on) of every window."""
    v = _windows(x)
    m = v[0].clone()
    arg = torch.zeros(m.shape, dtype=torch.int64)
    for q in (1, 2, 3):
        take = (v[q] > m) | v[q].isnan()
        m = torch.where(take, v[q], m)
        arg = torch.where(take, torch.full_like(arg, q), arg)
    return m, arg


def maxpool2_fwd(x):
    return maxpool2_scan(x)[0]


def take_by_arg(x, arg):
    """The window element number `arg` of every window of x (any dtype: used on the int16 bit patterns)."""
    v = _windows(x)
    out = v[0].clone()
    for q in (1, 2, 3):
        out = torch.where(arg == q, v[q], out)
    return out


def maxpool2_bwd(x, dy, relu_mask=False):
    m, arg = maxpool2_scan(x)
    oh, ow = m.shape[1], m.shape[2]
    keep = (m > 0) if relu_mask else torch.ones_like(m, dtype=torch.bool)
    dx = torch.zeros_like(x)
    for q, (i, j) in enumerate(SCAN):
        dx[:, i:2 * oh:2, j:2 * ow:2] = torch.where((arg == q) & keep, dy, torch.zeros_like(dy))
    return dx


def avgpool2_fwd(x):
    v = _windows(x)
    return (v[0] + v[1] + v[2] + v[3]) * 0.25, (v[0].abs() + v[1].abs() + v[2].abs() + v[3].abs()) * 0.25


def avgpool2_bwd(dy, h, w):
    n, oh, ow, c = dy.shape
    assert (oh, ow) == (h // 2, w // 2)
    dx = torch.zeros(n, h, w, c, dtype=torch.float64)
    for i, j in SCAN:
        dx[:, i:2 * oh:2, j:2 * ow:2] = dy * 0.25
    return dx


def nearest2x_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty(n, 2 * h, 2 * w, c, dtype=x.dtype)
    for i, j in SCAN:
        y[:, i::2, j::2] = x
    return y


def nearest2x_bwd(dy):
    v = [dy[:, i::2, j::2] for i, j in SCAN]
    return v[0] + v[1] + v[2] + v[3], v[0].abs() + v[1].abs() + v[2].abs() + v[3].abs()


# ----------------------------------------------------------------------------- bilinear x2
def bil_src(o, n_in):
    s = max(0.0, (o + 0.5) / 2 - 0.5)
    i0 = int(s)
    return i0, min(i0 + 1, n_in - 1), s - i0


def bil_matrix(n_in):
    """[2 n_in, n_in]: row o holds the two weights of output o (they share a column where the upper index is clamped)."""
    m = torch.zeros(2 * n_in, n_in, dtype=torch.float64)
    for o in range(2 * n_in):
        i0, i1, l = bil_src(o, n_in)
        m[o, i0] += 1.0 - l
        m[o, i1] += l
    return m


def _sep(my, mx, x):
    """out[n, p, q, c] = sum_hw my[p, h] mx[q, w] x[n, h, w, c]"""
    return torch.einsum("ph,qw,nhwc->npqc", my, mx, x)


def bilinear2x_fwd(x):
    my, mx = bil_matrix(x.shape[1]), bil_matrix(x.shape[2])
    return _sep(my, mx, x), _sep(my, mx, x.abs())


def bilinear2x_bwd(dy):
    my, mx = bil_matrix(dy.shape[1] // 2).t(), bil_matrix(dy.shape[2] // 2).t()
    return _sep(my, mx, dy), _sep(my, mx, dy.abs())


# ----------------------------------------------------------------------------- resize + crop + normalise from packed tables
def pack_tables(windows, kt):
    """[(start, fp32 weights)] -> (start int32 [O], count int32 [O], w fp32 [O, kt]), the layout the kernels read."""
    n = len(windows)
    s, c, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, kt), np.float32)
    for i, (st, ws) in enumerate(windows):
        assert len(ws) <= kt
        s[i], c[i] = st, len(ws)
        w[i, :len(ws)] = ws
    return s, c, w


def table_matrix(tab, in_size):
    """Packed tables -> dense [O, in_size] float64: M[o, start[o] + i] += w[o, i] for i < count[o]."""
    s, c, w = tab
    m = torch.zeros(len(s), in_size, dtype=torch.float64)
    for o in range(len(s)):
        for i in range(int(c[o])):
            m[o, int(s[o]) + i] += float(w[o, i])
    return m


def _chan(v, c):
    return torch.tensor(np.asarray(v, dtype=np.float32)[:c].astype(np.float64))


def resize_norm_fwd(src, ytab, xtab, mean, std):
    """src fp64 [N, C, H, W] -> ([N, OH, OW, 8], A).  mean / std: three fp32 values."""
    n, c, h, w = src.shape
    my, mx = table_matrix(ytab, h), table_matrix(xtab, w)
    mean, std = _chan(mean, c), _chan(std, c)
    acc = torch.einsum("ph,qw,nchw->npqc", my, mx, src)
    aacc = torch.einsum("ph,qw,nchw->npqc", my.abs(), mx.abs(), src.abs())
    out = torch.zeros(n, my.shape[0], mx.shape[0], 8, dtype=torch.float64)
    a = torch.zeros_like(out)
    out[..., :c] = (acc - mean) / std
    a[..., :c] = (aacc + mean.abs()) / std
    return out, a


def resize_norm_bwd(dout, tytab, txtab, std, c, h, w):
    """dout fp64 [N, OH, OW, 8] -> (dsrc [N, C, H, W], A) from the transposed tables (row = input index)."""
    oh, ow = dout.shape[1], dout.shape[2]
    ty, tx = table_matrix(tytab, oh), table_matrix(txtab, ow)
    assert ty.shape[0] == h and tx.shape[0] == w
    std = _chan(std, c).reshape(1, c, 1, 1)
    d = dout[..., :c]
    return (torch.einsum("hp,wq,npqc->nchw", ty, tx, d) / std,
            torch.einsum("hp,wq,npqc->nchw", ty.abs(), tx.abs(), d.abs()) / std)


# ----------------------------------------------------------------------------- box copy
def box_copy(src, dst, n, bh, bw, c, sy0, sx0, cs0, dy0, dx0, cd0):
    out = dst.clone()
    out[:n, dy0:dy0 + bh, dx0:dx0 + bw, cd0:cd0 + c] = src[:n, sy0:sy0 + bh, sx0:sx0 + bw, cs0:cs0 + c]
    return out


# ----------------------------------------------------------------------------- fixed-kernel downsampler
def ds_out(size, k, f, p):
    """Output extent; 0 where the padded input is smaller than the kernel."""
    return (size + 2 * p - k) // f + 1 if size + 2 * p >= k else 0


def _clamp_index(size, p):
    return torch.arange(-p, size + p).clamp(0, size - 1)


def downsample_fwd(x, kern, f, p):
    """x [NC, H, W], kern [k, k] -> (y [NC, OH, OW], A): explicit replicate pad, then the strided correlation."""
    nc, h, w = x.shape
    k = kern.shape[0]
    oh, ow = ds_out(h, k, f, p), ds_out(w, k, f, p)
    xp = x[:, _clamp_index(h, p)][:, :, _clamp_index(w, p)]
    y, a = torch.zeros(nc, oh, ow, dtype=torch.float64), torch.zeros(nc, oh, ow, dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            t = kern[i, j] * xp[:, i:i + f * (oh - 1) + 1:f, j:j + f * (ow - 1) + 1:f]
            y += t
            a += t.abs()
    return y, a


def downsample_bwd(dy, kern, h, w, f, p):
    """dy [NC, OH, OW] -> (dx [NC, H, W], A, largest number of terms any dx element sums)."""
    nc, oh, ow = dy.shape
    k = kern.shape[0]
    assert (oh, ow) == (ds_out(h, k, f, p), ds_out(w, k, f, p))
    outs = []
    for d, kk in ((dy, kern), (dy.abs(), kern.abs()), (torch.ones_like(dy[:1]), torch.ones_like(kern))):
        dxp = torch.zeros(d.shape[0], h + 2 * p, w + 2 * p, dtype=torch.float64)
        for i in range(k):
            for j in range(k):
                dxp[:, i:i + f * (oh - 1) + 1:f, j:j + f * (ow - 1) + 1:f] += kk[i, j] * d
        t = torch.zeros(d.shape[0], h, w + 2 * p, dtype=torch.float64).index_add_(1, _clamp_index(h, p), dxp)
        outs.append(torch.zeros(d.shape[0], h, w, dtype=torch.float64).index_add_(2, _clamp_index(w, p), t))
    return outs[0], outs[1], int(outs[2].max())


# ============================================================================= case tables
NS = (1, 3)
CPS = (8, 24, 40)                     # 1, 3 and 5 channel groups per pixel
HWS = ((2, 2), (2, 3), (3, 2), (5, 7), (7, 10), (16, 18))
THIN_HWS = ((1, 1), (1, 5), (4, 1))   # the two upsamplers and the average-pool adjoint also take H = 1 or W = 1


def shapes(thin=False):
    return [(n, h, w, cp) for n in NS for cp in CPS for (h, w) in (HWS + THIN_HWS if thin else HWS)]


def kernel_threads():
    """Thread count of every launch of the pool / upsampler sweep, per kernel (one thread per 8-channel group of the side the
    kernel walks)."""
    t = {}
    for n, h, w, cp in shapes():
        g = cp // 8
        t.setdefault("maxpool2_fwd", []).append(n * (h // 2) * (w // 2) * g)
        t.setdefault("maxpool2_bwd", []).append(n * h * w * g)
        t.setdefault("avgpool2_fwd", []).append(n * (h // 2) * (w // 2) * g)
    for n, h, w, cp in shapes(thin=True):
        g = cp // 8
        t.setdefault("avgpool2_bwd", []).append(n * h * w * g)
        for name in ("nearest2x_fwd", "bilinear2x_fwd"):
            t.setdefault(name, []).append(4 * n * h * w * g)
        for name in ("nearest2x_bwd", "bilinear2x_bwd"):
            t.setdefault(name, []).append(n * h * w * g)
    return t


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(v) for v in key))) % (2 ** 31))


def grid(gen, shape, step, amp):
    """Multiples of `step` in [-amp, amp], float64."""
    return (torch.randint(-(amp // step), amp // step + 1, shape, generator=gen) * step).to(torch.float64)


# +Inf, -Inf, two NaNs with payloads, both zeros, the smallest subnormal and the largest negative one
SPECIAL_BITS = {BF16: (0x7F80, 0xFF80, 0x7FC1, 0xFFA5, 0x0000, 0x8000, 0x0001, 0x807F),
                F16: (0x7C00, 0xFC00, 0x7E01, 0xFD55, 0x0000, 0x8000, 0x0001, 0x83FF)}


def bits16(gen, shape, dtype):
    """Arbitrary 16-bit patterns as int16, with SPECIAL_BITS planted at every 13th element."""
    t = torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32).reshape(-1)
    sp = torch.tensor(SPECIAL_BITS[dtype], dtype=torch.int32)
    sp = torch.where(sp >= 32768, sp - 65536, sp)
    idx = torch.arange(0, t.numel(), 13)
    t[idx] = sp[torch.arange(len(idx)) % len(sp)]
    return t.to(torch.int16).reshape(shape)


def real16(gen, shape, dtype):
    """N(0,1) rounded to the storage type, float64."""
    return r16(torch.randn(shape, generator=gen, dtype=torch.float64), dtype)


# exact-regime grids (step, largest magnitude): inputs / output gradients of each op
BIL_GRID = (16, 48)          # weights are multiples of 1/16: outputs are integers <= 48, gradients integers <= 4 * 48
AVG_GRID = (4, 60)           # the mean of four multiples of 4 is an integer <= 60; dy / 4 likewise
NEAREST_GRID = (1, 15)       # sums of four stay <= 60


@functools.lru_cache(maxsize=None)
def exact_case(n, h, w, cp):
    """Exact-regime inputs of one shape and their float64 references (computed once; do not modify)."""
    g = _gen(1, n, h, w, cp)
    d = dict(shape=(n, h, w, cp))
    up, low = (n, 2 * h, 2 * w, cp), (n, h // 2, w // 2, cp)
    d["bil_x"], d["bil_dy"] = grid(g, (n, h, w, cp), *BIL_GRID), grid(g, up, *BIL_GRID)
    d["bil_y"], d["bil_dx"] = bilinear2x_fwd(d["bil_x"])[0], bilinear2x_bwd(d["bil_dy"])[0]
    d["near_dy"] = grid(g, up, *NEAREST_GRID)
    d["near_dx"] = nearest2x_bwd(d["near_dy"])[0]
    d["avg_x"], d["avg_dy"] = grid(g, (n, h, w, cp), *AVG_GRID), grid(g, low, *AVG_GRID)
    d["avg_dx"] = avgpool2_bwd(d["avg_dy"], h, w)
    if h >= 2 and w >= 2:
        d["avg_y"] = avgpool2_fwd(d["avg_x"])[0]
        # max pool on small integers: plenty of ties; the gradient is any representable integer
        d["max_x"], d["max_dy"] = grid(g, (n, h, w, cp), 1, 3), grid(g, low, 1, 60)
        d["max_dx"] = maxpool2_bwd(d["max_x"], d["max_dy"])
        d["relu_x"] = d["max_x"].clamp_min(0)
        d["relu_dx"] = maxpool2_bwd(d["relu_x"], d["max_dy"], relu_mask=True)
    return d


# ---- max-pool edge windows: (v00, v01, v10, v11) -> every window's winner follows from the rule in the docstring
MAXPOOL_EDGES = [
    (NAN, 1, 2, 3), (1, NAN, 2, 3), (1, 2, NAN, 3), (3, 2, 1, NAN),                      # a NaN at each position
    (NAN, NAN, 1, 2), (NAN, 1, 2, NAN), (1, NAN, NAN, 2), (1, 2, NAN, NAN), (NAN, 5, NAN, 1), (NAN, NAN, NAN, NAN),
    (INF, 1, 2, 3), (1, 2, INF, 3), (-INF, 1, 2, 3), (1, -INF, -INF, -INF), (-INF, -INF, -INF, -INF),
    (INF, INF, 1, 2), (1, INF, 2, INF), (INF, NAN, 1, 2), (NAN, INF, 1, 2), (-INF, NAN, -INF, -INF), (INF, -INF, INF, -INF),
    (2, 2, 2, 2), (0, 0, 0, 0), (-3, -3, -3, -3), (-0.0, 0.0, 0.0, -0.0), (0.0, -0.0, -0.0, 0.0),     # all-equal windows
    (5, 5, 1, 2), (5, 1, 5, 2), (5, 1, 2, 5), (1, 5, 5, 2), (1, 5, 2, 5), (1, 2, 5, 5), (1, 5, 5, 5),  # ties: the first one wins
    (-1, -2, -1, -2), (57344.0, 57344.0, -57344.0, 1), (1, 2, 3, 4), (4, 3, 2, 1),
]
# windows of a ReLU output (finite and non-negative, or +Inf) for the ReLU-masked backward
RELU_EDGES = [(0, 0, 0, 0), (INF, 1, 2, 3), (1, 2, 3, INF), (INF, INF, 0, 0), (0, 0, 0, 7), (2, 2, 2, 2), (0, 3, 3, 0),
              (0, 0, 5, 5), (1, 0, 0, 1), (0, 57344.0, 57344.0, 0), (0.5, 0.25, 0, 0), (0, 0, 0.0078125, 0)]
EDGE_DY = [7.0, INF, -3.0, NAN, 0.5, -INF, 11.0, 1.0]      # the gradient values dealt over the windows


def edge_case(windows):
    """x [2, 3, 2 K + 1, 8] holding every window of `windows` once per channel lane and image (lane c of image n holds window
    (k + 3 c + 5 n) % K at position k, so the eight lanes of a vector never agree); row 2 and the last column are the
    trailing odd ones and hold +Inf, which a pool that read them would pick.  dy deals EDGE_DY."""
    k = len(windows)
    t = torch.tensor(windows, dtype=torch.float64)
    x = torch.full((2, 3, 2 * k + 1, 8), INF, dtype=torch.float64)
    dy = torch.empty(2, 1, k, 8, dtype=torch.float64)
    for n in range(2):
        for c in range(8):
            for pos in range(k):
                win = t[(pos + 3 * c + 5 * n) % k]
                x[n, 0, 2 * pos, c], x[n, 0, 2 * pos + 1, c], x[n, 1, 2 * pos, c], x[n, 1, 2 * pos + 1, c] = win
                dy[n, 0, pos, c] = EDGE_DY[(pos + c + n) % len(EDGE_DY)]
    return x, dy


# ---- resize + normalise: hand-built tables
RESIZE_H, RESIZE_W = 16, 50                       # N * H * W = 1600 backward threads: above 256 and no multiple of it
RESIZE_XCOUNTS = (1, 15, 16, 17, 40) * 3          # both sides of the kernel's nx <= 16 branch and its boundary, in one launch
RESIZE_YCOUNTS = (9, 1) * 5                       # N * OH * OW = 300 forward threads
RESIZE_MEAN = (0.485, 0.456, 0.406)
RESIZE_STD = (0.229, 0.224, 0.225)


def _hand_windows(rng, counts, in_size):
    out = []
    for c in counts:
        start = int(rng.integers(0, in_size - c + 1))
        w = (rng.random(c) + 0.25)
        out.append((start, (w / w.sum()).astype(np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def resize_family():
    """(row windows, column windows) of the hand-built family: lists of (start, fp32 weights that differ in every row)."""
    rng = np.random.default_rng(20240607)
    return _hand_windows(rng, RESIZE_YCOUNTS, RESIZE_H), _hand_windows(rng, RESIZE_XCOUNTS, RESIZE_W)


def identity_windows(size):
    """No resampling: every output is its input with one weight of 1."""
    return [(i, np.ones(1, dtype=np.float32)) for i in range(size)]


# ---- box copy: (N, BH, BW, C, SH, SW, SCp, sy0, sx0, cs0, DH, DW, DCp, dy0, dx0, cd0)
BOX_CASES = [
    (2, 3, 5, 13, 7, 9, 24, 2, 3, 5, 6, 8, 40, 1, 2, 19),          # every offset nonzero, C no multiple of 8
    (1, 8, 8, 4, 10, 12, 8, 1, 2, 0, 8, 8, 24, 0, 0, 0),            # Concat's centre crop of the first branch
    (1, 8, 8, 13, 8, 8, 16, 0, 0, 0, 8, 8, 24, 0, 0, 4),            # ... and the second branch behind it
    (3, 16, 11, 17, 16, 11, 24, 0, 0, 7, 18, 12, 24, 2, 1, 3),      # 8976 threads: 35 blocks and a part of one
    (1, 1, 1, 1, 1, 1, 8, 0, 0, 7, 1, 1, 8, 0, 0, 0),
]
# one argument of the first case pushed so that the box leaves the source or the destination: (index, value)
BOX_OUTSIDE = [(7, 5), (8, 5), (9, 12), (13, 4), (14, 4), (15, 28), (7, -1), (14, -1), (1, 8), (2, 9)]

# ---- downsampler
DS_K, DS_F = (3, 4, 8), (1, 2, 3, 4)
DS_HW = ((1, 1), (1, 5), (2, 13), (5, 2), (5, 9), (9, 1), (9, 13), (13, 5), (13, 13))      # 1, 2, 5, 9, 13 on either axis
DS_NC = 3


def ds_cases():
    """(k, f, p, H, W) with a non-empty output."""
    out = []
    for k in DS_K:
        for f in DS_F:
            for p in sorted({0, 1, k // 2}):
                for h, w in DS_HW:
                    if ds_out(h, k, f, p) >= 1 and ds_out(w, k, f, p) >= 1:
                        out.append((k, f, p, h, w))
    return out


# padded input smaller than the kernel: an error, also where C's truncating division would make (H + 2p - k) / f + 1 == 1
DS_EMPTY = [(3, 1, 0, 1, 1), (3, 4, 0, 1, 5), (8, 3, 1, 5, 9), (8, 4, 0, 13, 5), (4, 2, 1, 1, 13), (4, 4, 0, 2, 13)]


@functools.lru_cache(maxsize=None)
def ds_kernel(k):
    """A non-symmetric k x k fp32 kernel (a transposed i / j shows), as float64."""
    g = _gen(7, k)
    return torch.randn(k, k, generator=g, dtype=torch.float32).to(torch.float64)
