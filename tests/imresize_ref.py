"""Float64 yardstick of the MATLAB-style imresize, written in loop form from its definition and independent of the product's
table builder (utils/imresize.py).

Per axis, input length n, scale s (given, output length m = ceil(s n); or s = m / n for a given m).  Kernel k of width kw:
bicubic (a = -0.5, kw 4), bilinear (triangle, kw 2), lanczos2 / lanczos3 (sinc(x) sinc(x / a) for |x| < a, kw 2 a).  With
antialiasing and s < 1: h(x) = s k(s x), kw <- kw / s; otherwise h = k.  For the 1-based output o:
    u = o / s + 0.5 (1 - 1 / s);  left = floor(u - kw / 2);  P = ceil(kw) + 2 taps at positions left .. left + P - 1,
    weights h(u - position) divided by their sum;  positions mirrored with the edge pixel repeated (period 2 n: 1..n, n..1,
    1..n, ...);  tap columns that are zero for every output are dropped.
The 2-D result is the two 1-D passes, the axis with the smaller scale first (MATLAB's order).  Parity with MATLAB itself is
unpinned; the independent cross-check is torch's antialiased bicubic in the interior (tests/test_host_imresize.py)."""
import math

import numpy as np

KW = {"bicubic": 4.0, "bilinear": 2.0, "lanczos2": 4.0, "lanczos3": 6.0}


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def kernel_value(kernel, x):
    ax = abs(x)
    if kernel == "bicubic":
        if ax <= 1.0:
            return 1.5 * ax * ax * ax - 2.5 * ax * ax + 1.0
        if ax <= 2.0:
            return -0.5 * ax * ax * ax + 2.5 * ax * ax - 4.0 * ax + 2.0
        return 0.0
    if kernel == "bilinear":
        return 1.0 - ax if ax <= 1.0 else 0.0
    a = {"lanczos2": 2.0, "lanczos3": 3.0}[kernel]
    return _sinc(x) * _sinc(x / a) if ax < a else 0.0


def out_len(n_in, scale):
    return int(math.ceil(scale * n_in))


def contributions(n_in, n_out, scale, kernel="bicubic", antialiasing=True):
    """(weights float64 [n_out, taps], indices int64 [n_out, taps]: 0-based, mirrored)."""
    kw = KW[kernel]
    s = float(scale)
    shrink = antialiasing and s < 1.0
    if shrink:
        kw = kw / s
    p = int(math.ceil(kw)) + 2
    weights = np.zeros((n_out, p), dtype=np.float64)
    indices = np.zeros((n_out, p), dtype=np.int64)
    for o in range(1, n_out + 1):
        u = o / s + 0.5 * (1.0 - 1.0 / s)
        left = math.floor(u - kw / 2.0)
        row = []
        for j in range(p):
            pos = left + j
            x = u - pos
            row.append(s * kernel_value(kernel, s * x) if shrink else kernel_value(kernel, x))
            q = (pos - 1) % (2 * n_in)                       # 0-based position within one mirror period
            indices[o - 1, j] = q if q < n_in else 2 * n_in - 1 - q
        total = 0.0
        for v in row:
            total += v
        for j in range(p):
            weights[o - 1, j] = row[j] / total
    keep = [j for j in range(p) if any(weights[o, j] != 0.0 for o in range(n_out))]
    return weights[:, keep].copy(), indices[:, keep].copy()


def _plan(h, w, scale, size):
    if scale is not None:
        sh, sw = scale if isinstance(scale, (tuple, list)) else (scale, scale)
        return (out_len(h, sh), float(sh)), (out_len(w, sw), float(sw))
    return (int(size[0]), size[0] / h), (int(size[1]), size[1] / w)


def _apply(x, weights, indices, axis):
    """One pass along `axis` of a float64 array: y[o] = sum_t weights[o, t] x[indices[o, t]], taps added in tap order."""
    x = np.moveaxis(x, axis, 0)
    out = np.zeros((weights.shape[0],) + x.shape[1:], dtype=x.dtype)
    for o in range(weights.shape[0]):
        for t in range(weights.shape[1]):
            out[o] = out[o] + weights[o, t].astype(x.dtype) * x[indices[o, t]]
    return np.moveaxis(out, 0, axis)


def _apply_adjoint(dy, weights, indices, n_in, axis):
    dy = np.moveaxis(dy, axis, 0)
    out = np.zeros((n_in,) + dy.shape[1:], dtype=dy.dtype)
    for o in range(weights.shape[0]):
        for t in range(weights.shape[1]):
            out[indices[o, t]] = out[indices[o, t]] + weights[o, t] * dy[o]
    return np.moveaxis(out, 0, axis)


def _axis_tables(x_shape, scale, size, kernel, antialiasing, tables):
    h, w = x_shape[-2], x_shape[-1]
    (oh, sh), (ow, sw) = _plan(h, w, scale, size)
    if tables is None:
        tables = (contributions(h, oh, sh, kernel, antialiasing), contributions(w, ow, sw, kernel, antialiasing))
    return tables, sh, sw


def resize(x, scale=None, size=None, kernel="bicubic", antialiasing=True, tables=None):
    """float64 [..., H, W] -> [..., OH, OW].  `tables` = ((w_h, idx_h), (w_w, idx_w)) replaces the contributions, e.g. by the
    product's fp32-rounded weights (a comparison against that covers the accumulation only)."""
    x = np.asarray(x, dtype=np.float64)
    (th, tw), sh, sw = _axis_tables(x.shape, scale, size, kernel, antialiasing, tables)
    order = [(-2, th), (-1, tw)] if sh <= sw else [(-1, tw), (-2, th)]
    for axis, (wt, idx) in order:
        x = _apply(x, np.asarray(wt, dtype=np.float64), idx, axis)
    return x


def adjoint(dy, in_hw, scale=None, size=None, kernel="bicubic", antialiasing=True, tables=None):
    """The transpose of ``resize`` for an input of in_hw = (H, W): float64 [..., OH, OW] -> [..., H, W]."""
    dy = np.asarray(dy, dtype=np.float64)
    (th, tw), _, _ = _axis_tables(tuple(dy.shape[:-2]) + tuple(in_hw), scale, size, kernel, antialiasing, tables)
    dy = _apply_adjoint(dy, np.asarray(th[0], dtype=np.float64), th[1], in_hw[0], -2)
    return _apply_adjoint(dy, np.asarray(tw[0], dtype=np.float64), tw[1], in_hw[1], -1)


def fp32_emulation(x, scale=None, size=None, kernel="bicubic", antialiasing=True, tables=None):
    """The device's two passes (H, then W) in numpy float32 with a separately rounded multiply and add per tap: every step
    rounds at least as often as the kernel's fmaf, so what this loses bounds what the kernel can lose, and where this is exact
    the kernel is."""
    x = np.asarray(x, dtype=np.float32)
    (th, tw), _, _ = _axis_tables(x.shape, scale, size, kernel, antialiasing, tables)
    x = _apply(x, np.asarray(th[0], dtype=np.float64).astype(np.float32), th[1], -2)
    return _apply(x, np.asarray(tw[0], dtype=np.float64).astype(np.float32), tw[1], -1)


def fp32_adjoint_emulation(dy, in_hw, scale=None, size=None, kernel="bicubic", antialiasing=True, tables=None):
    """``adjoint`` the way the device runs it (H, then W; per source pixel ascending in the output, then in tap order) in
    numpy float32 with separately rounded multiplies and adds."""
    dy = np.asarray(dy, dtype=np.float32)
    (th, tw), _, _ = _axis_tables(tuple(dy.shape[:-2]) + tuple(in_hw), scale, size, kernel, antialiasing, tables)
    dy = _apply_adjoint(dy, np.asarray(th[0], dtype=np.float64).astype(np.float32), th[1], in_hw[0], -2)
    return _apply_adjoint(dy, np.asarray(tw[0], dtype=np.float64).astype(np.float32), tw[1], in_hw[1], -1)


def row_abs_sum(weights):
    """A of the error bound: the largest row sum of |w|."""
    return float(np.abs(np.asarray(weights, dtype=np.float64)).sum(axis=1).max())


def quantise_u8(v):
    return np.clip(np.floor(np.asarray(v, dtype=np.float64) + 0.5), 0, 255).astype(np.uint8)


# ----------------------------------------------------------------------------- cases shared by the host and the GPU tests
# Exact configurations: every weight is dyadic and, with integer inputs of the given range, every partial sum fits 24 bits,
# so fp32 accumulation in any order equals float64.  (kernel, scale, largest input value, largest dy value)
EXACT_CONFIGS = [("bilinear", 0.5, 255, 255), ("bilinear", 0.25, 255, 255), ("bilinear", 2, 255, 255), ("bilinear", 4, 255, 255),
                 ("bicubic", 2, 255, 15), ("bicubic", 0.5, 31, 15)]
# (shape, kernel, scale, input range, dy range): (2,3,37,53) for every configuration; an input shorter than the support; a
# shape that crosses tile edges in both axes; a tiny upscale; a wide strip
EXACT_CASES = ([((2, 3, 37, 53), k, s, hi, dhi) for k, s, hi, dhi in EXACT_CONFIGS] +
               [((1, 1, 5, 7), "bilinear", 0.25, 255, 255), ((1, 3, 130, 260), "bilinear", 0.25, 255, 255),
                ((1, 1, 9, 11), "bilinear", 4, 255, 255),
                # three tiles along W whose strips (31 * 8 + 16 columns) are wider than one sweep of a wave's 256 columns
                ((1, 1, 24, 600), "bilinear", 0.125, 255, 255)])


def exact_input(shape, hi, seed=0):
    """Seeded integer-valued float64 array with values 0..hi."""
    return np.random.RandomState(seed).randint(0, hi + 1, size=shape).astype(np.float64)


U8_SHAPE = (61, 47, 3)
U8_SEED = 0


def u8_image(seed=U8_SEED, shape=U8_SHAPE):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def resize_hwc(img, **kw):
    """``resize`` of an [H, W, C] array (float64 result, unrounded)."""
    return np.moveaxis(resize(np.moveaxis(np.asarray(img, dtype=np.float64), 2, 0), **kw), 0, 2)
