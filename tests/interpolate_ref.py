"""Float64 yardstick of utils.imresize.interpolate: torch.nn.functional.interpolate on the CPU in float64 (align_corners=False,
no antialias), and the loop form of the definition written out per axis.  Nothing here comes from the product."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MODES = ("area", "bilinear", "bicubic")
SCALES = (0.15, 0.3, 0.5, 0.77, 1.0, 1.2, 1.5)
SIZES = ((17, 23), (40, 33), (64, 64))


def torch_interpolate(x, size=None, scale_factor=None, mode="bilinear"):
    """float64 F.interpolate; x: [N, C, H, W] (array or tensor) -> float64 tensor"""
    x = torch.as_tensor(x).double()
    kw = {} if mode == "area" else {"align_corners": False}
    return F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, **kw)


def out_size(n, size=None, scale_factor=None):
    return int(size) if size is not None else int(math.floor(float(n) * float(scale_factor)))


def _cc1(x, a):
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0


def _cc2(x, a):
    return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a


def axis_matrix(n_in, n_out, mode, scale_factor=None):
    """The loop form: float64 [n_out, n_in] matrix of one axis."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    rho = 1.0 / scale_factor if scale_factor is not None else n_in / n_out
    for o in range(n_out):
        if mode == "area":
            lo = int(math.floor(o * n_in / n_out))
            hi = int(math.ceil((o + 1) * n_in / n_out))
            for i in range(lo, hi):
                m[o, i] += 1.0 / (hi - lo)
        elif mode == "bilinear":
            s = max((o + 0.5) * rho - 0.5, 0.0)
            i0 = int(math.floor(s))
            lam = s - i0
            m[o, i0] += 1.0 - lam
            m[o, min(i0 + 1, n_in - 1)] += lam
        else:
            s = (o + 0.5) * rho - 0.5
            i0 = int(math.floor(s))
            t = s - i0
            for d, wt in zip((-1, 0, 1, 2), (_cc2(t + 1.0, -0.75), _cc1(t, -0.75), _cc1(1.0 - t, -0.75), _cc2(2.0 - t, -0.75))):
                m[o, min(max(i0 + d, 0), n_in - 1)] += wt
    return m


def loop_interpolate(x, size=None, scale_factor=None, mode="bilinear"):
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[-2:]
    sh, sw = (None, None) if scale_factor is None else (scale_factor, scale_factor)
    oh = out_size(h, None if size is None else size[0], sh)
    ow = out_size(w, None if size is None else size[1], sw)
    mh, mw = axis_matrix(h, oh, mode, sh), axis_matrix(w, ow, mode, sw)
    return np.einsum("oh,nchw,pw->ncop", mh, x, mw)


def apply_tables(x, tables_h, tables_w):
    """x through per-axis (weights [out, taps], indices [out, taps]) tables in numpy float64: H pass, then W pass"""
    x = np.asarray(x, dtype=np.float64)
    (wh, ih), (ww, iw) = tables_h, tables_w
    t = np.einsum("ot,ncotw->ncow", wh, x[:, :, ih, :])
    return np.einsum("pt,ncopt->ncop", ww, t[:, :, :, iw])


def row_abs_sum(w):
    return float(np.abs(np.asarray(w, dtype=np.float64)).sum(axis=1).max())
