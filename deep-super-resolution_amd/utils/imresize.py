"""MATLAB-style antialiased ``imresize`` on the device (csrc/imresize.hip), differentiable with respect to a float image.

How every super-resolution benchmark makes its low-resolution set (DIV2K ``LR_bicubic``, Set5 / Set14 / B100 / Urban100):
``imresize(hr, 1 / s, 'bicubic')`` -- a cubic kernel with a = -0.5, widened by 1 / s against aliasing, weights normalised per
output pixel, borders mirrored.  Per axis (input length n, scale s, output length m = ceil(s n), or s = m / n for a given m),
for the 1-based output o:  u = o / s + 0.5 (1 - 1 / s);  left = floor(u - kw / 2);  P = ceil(kw) + 2 taps at left .. left + P - 1
with weights h(u - position) / their sum, h(x) = s k(s x) and kw = (kernel width) / s when antialiasing shrinks, else h = k;
positions mirror with the edge pixel repeated (period 2 n);  tap columns that are zero for every output are dropped.  All of it
in float64 on the host, rounded to fp32 once; the device then runs one fmaf per tap in tap order, H pass then W pass, with no
rounding in between -- the uint8 entry computes in fp32 from the bytes and stores ``min(max(floorf(v + 0.5f), 0), 255)`` once.

Parity with MATLAB itself is unpinned (no MATLAB was available): its uint8 path may round between the two passes, which this
one does not.  The float64 statement of the definition above is tests/imresize_ref.py; the interior of its output equals
``torch.nn.functional.interpolate(mode='bicubic', antialias=True)``, the borders differ (torch truncates, this mirrors).

Limits: 64 taps per axis (bicubic down to about 1/15, lanczos3 to 1/10; more raises NotImplementedError), and
planes * max(H W, OH OW) < 2^31.
"""
import math

import numpy as np
import torch

from .. import _lib
from .. import functional as F
from ..functional import _need_gpu, _ptr, _stream
from .degradation import _to_device

MAX_TAPS = 64
_cache = {}


def _cubic(x):
    ax = np.abs(x)
    ax2 = ax * ax
    ax3 = ax2 * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1.0) * (ax <= 1.0) + (-0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0) * ((ax > 1.0) & (ax <= 2.0))


def _triangle(x):
    ax = np.abs(x)
    return (1.0 - ax) * (ax <= 1.0)


def _lanczos(a):
    def k(x):
        ax = np.abs(x)
        px = np.pi * np.where(ax == 0.0, 1.0, ax)
        v = np.sin(px) * np.sin(px / a) * a / (px * px)
        return np.where(ax == 0.0, 1.0, v) * (ax < a)
    return k


KERNELS = {"bicubic": (_cubic, 4.0), "bilinear": (_triangle, 2.0), "lanczos2": (_lanczos(2.0), 4.0), "lanczos3": (_lanczos(3.0), 6.0)}


def _check_kernel(kernel):
    if kernel not in KERNELS:
        raise ValueError(f"imresize: unknown kernel {kernel!r}; one of {sorted(KERNELS)}")


def axis_weights(n_in, n_out, scale, kernel="bicubic", antialiasing=True):
    """Host float64 (weights [n_out, taps], 0-based mirrored indices int64 [n_out, taps]) of one axis."""
    _check_kernel(kernel)
    k, kw = KERNELS[kernel]
    s = float(scale)
    shrink = bool(antialiasing) and s < 1.0
    if shrink:
        kw = kw / s
    o = np.arange(1, n_out + 1, dtype=np.float64)
    u = o / s + 0.5 * (1.0 - 1.0 / s)
    left = np.floor(u - kw / 2.0)
    p = int(math.ceil(kw)) + 2
    pos = left[:, None] + np.arange(p, dtype=np.float64)[None, :]
    d = u[:, None] - pos
    w = s * k(s * d) if shrink else k(d)
    total = np.zeros(n_out, dtype=np.float64)
    for j in range(p):                      # tap order, like the loop form of the definition
        total = total + w[:, j]
    w = w / total[:, None]
    idx = np.mod(pos.astype(np.int64) - 1, 2 * n_in)
    idx = np.where(idx < n_in, idx, 2 * n_in - 1 - idx)
    keep = np.any(w != 0.0, axis=0)
    return np.ascontiguousarray(w[:, keep]), np.ascontiguousarray(idx[:, keep])


class AxisTables:
    """Device tables of one axis.  Forward: ``idx`` int32 / ``w`` fp32 [n_out, taps].  Transposed: ``t_idx`` / ``t_w``
    [n_in, q] -- for source i the (output, weight) pairs that read it, ascending in the output and then in tap order (pairs
    whose fp32 weight is 0 are left out), padded to the longest list ``q`` with weight 0 and a neighbouring output."""

    def __init__(self, n_in, n_out, scale, w64, idx, device):
        self.n_in, self.n_out, self.scale = n_in, n_out, scale
        w32 = w64.astype(np.float32)
        self.taps = int(w32.shape[1])
        lists = [[] for _ in range(n_in)]
        for o in range(n_out):
            for t in range(self.taps):
                if w32[o, t] != 0.0:
                    lists[int(idx[o, t])].append((o, w32[o, t]))
        self.q = max(1, max(len(l) for l in lists))
        t_idx = np.zeros((n_in, self.q), dtype=np.int32)
        t_w = np.zeros((n_in, self.q), dtype=np.float32)
        for i, l in enumerate(lists):
            t_idx[i, :] = l[-1][0] if l else min(n_out - 1, i * n_out // n_in)
            for j, (o, v) in enumerate(l):
                t_idx[i, j], t_w[i, j] = o, v
        up = lambda a: torch.from_numpy(a).to(device)
        self.idx, self.w = up(idx.astype(np.int32)), up(w32)
        self.t_idx, self.t_w = up(t_idx), up(t_w)


def imresize_tables(n_in, n_out, scale, kernel="bicubic", antialiasing=True, device="cuda:0"):
    """The ``AxisTables`` (forward and transposed) of one axis on `device`, cached per argument tuple: float64 host arithmetic,
    one rounding to fp32, one upload."""
    _check_kernel(kernel)
    key = (int(n_in), int(n_out), float(scale), kernel, bool(antialiasing), str(device))
    hit = _cache.get(key)
    if hit is None:
        if n_in < 1 or n_out < 1 or not scale > 0:
            raise ValueError(f"imresize: axis of {n_in} -> {n_out} pixels at scale {scale}")
        w64, idx = axis_weights(key[0], key[1], key[2], kernel, key[4])
        hit = _cache[key] = AxisTables(key[0], key[1], key[2], w64, idx, device)
    return hit


def _plan(h, w, scale, size):
    """((OH, s_h), (OW, s_w)) from exactly one of `scale` (float or pair) and `size` (OH, OW)."""
    if (scale is None) == (size is None):
        raise ValueError("imresize: exactly one of `scale` and `size` is expected")
    if scale is not None:
        sh, sw = (scale if isinstance(scale, (tuple, list)) else (scale, scale))
        sh, sw = float(sh), float(sw)
        if not (sh > 0 and sw > 0):
            raise ValueError(f"imresize: scale {scale!r} is not positive")
        return (int(math.ceil(sh * h)), sh), (int(math.ceil(sw * w)), sw)
    oh, ow = (int(v) for v in size)
    if oh < 1 or ow < 1:
        raise ValueError(f"imresize: size {size!r}")
    return (oh, oh / h), (ow, ow / w)


def _tables(h, w, scale, size, kernel, antialiasing, device):
    _check_kernel(kernel)
    (oh, sh), (ow, sw) = _plan(h, w, scale, size)
    return (imresize_tables(h, oh, sh, kernel, antialiasing, device), imresize_tables(w, ow, sw, kernel, antialiasing, device))


def imresize(x, scale=None, size=None, kernel="bicubic", antialiasing=True):
    """MATLAB-style ``imresize`` (see the module docstring).  Exactly one of ``scale`` (a float, or ``(s_h, s_w)``; the output
    is ``ceil(s n)`` long) and ``size`` = ``(OH, OW)``.  kernel: "bicubic", "bilinear", "lanczos2" or "lanczos3".

    A floating-point ``[N, C, H, W]`` device tensor goes through ``functional.Imresize``: fp32 out, differentiable with
    respect to `x`, one launch forward and one backward (anything but contiguous fp32 is made ``.contiguous().float()``).
    A uint8 ``[H, W, C]`` device tensor, numpy array or PIL image goes through dsr_imresize_u8 and comes back in its own type.
    MATLAB's own uint8 rounding between the passes is unpinned; this path rounds once, at the end."""
    if torch.is_tensor(x) and x.is_floating_point():
        if x.dim() != 4:
            raise TypeError(f"imresize: a float image must be [N, C, H, W], got {tuple(x.shape)}")
        _check_kernel(kernel)
        _plan(x.shape[2], x.shape[3], scale, size)          # argument errors come before the missing device
        _need_gpu(x)
        th, tw = _tables(x.shape[2], x.shape[3], scale, size, kernel, antialiasing, x.device)
        return F.Imresize.apply(x, th, tw)
    _check_kernel(kernel)
    if (scale is None) == (size is None):
        raise ValueError("imresize: exactly one of `scale` and `size` is expected")
    img, restore = _to_device(x)
    h, w, c = (int(v) for v in img.shape)
    th, tw = _tables(h, w, scale, size, kernel, antialiasing, img.device)
    out = torch.empty((th.n_out, tw.n_out, c), dtype=torch.uint8, device=img.device)
    F.imresize_check(_lib.lib().dsr_imresize_u8(_ptr(img), _ptr(out), h, w, c, th.n_out, tw.n_out, _ptr(th.idx), _ptr(th.w),
                                                th.taps, _ptr(tw.idx), _ptr(tw.w), tw.taps, _stream()))
    return restore(out)


# ------------------------------------------------------------------ torch-convention resize on the same kernel
INTERPOLATE_MODES = ("area", "bilinear", "bicubic")


def _cubic_torch(t, a=-0.75):
    """the four weights of torch's bicubic (a = -0.75) for the fraction t, taps floor(s) - 1 .. floor(s) + 2"""
    def near(x):
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0

    def far(x):
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return np.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], axis=1)


def interpolate_out_size(n_in, size=None, scale_factor=None):
    """Output length of one axis: `size` itself, or ``floor(n_in * scale_factor)`` computed in float64 as torch does."""
    if (size is None) == (scale_factor is None):
        raise ValueError("interpolate: exactly one of `size` and `scale_factor` is expected")
    n_out = int(size) if size is not None else int(math.floor(float(n_in) * float(scale_factor)))
    if n_out < 1:
        raise ValueError(f"interpolate: an axis of {n_in} pixels would become {n_out} long")
    return n_out


def interpolate_axis_weights(n_in, n_out, mode, scale_factor=None):
    """Host float64 (weights [n_out, taps], indices int64 [n_out, taps]) of one axis of ``torch.nn.functional.interpolate``
    with ``align_corners=False`` and no antialias.  The coordinate ratio is rho = n_in / n_out, or 1 / scale_factor when one is
    given (torch with ``recompute_scale_factor=None``).
      area      output o averages the sources floor(o n_in / n_out) .. ceil((o + 1) n_in / n_out) - 1 with equal weights
                (shorter lists are padded with weight 0);
      bilinear  s = max((o + 1/2) rho - 1/2, 0), taps floor(s) and min(floor(s) + 1, n_in - 1), weights 1 - l and l;
      bicubic   s = (o + 1/2) rho - 1/2 (not clamped), the cubic with a = -0.75 on taps floor(s) - 1 .. floor(s) + 2, indices
                clamped to the axis."""
    if mode not in INTERPOLATE_MODES:
        raise ValueError(f"interpolate: unknown mode {mode!r}; one of {INTERPOLATE_MODES}")
    o = np.arange(n_out, dtype=np.int64)
    if mode == "area":
        start = (o * n_in) // n_out
        end = -((-(o + 1) * n_in) // n_out)
        taps = int((end - start).max())
        t = np.arange(taps, dtype=np.int64)[None, :]
        live = t < (end - start)[:, None]
        w = np.where(live, 1.0 / (end - start)[:, None].astype(np.float64), 0.0)
        idx = np.minimum(start[:, None] + t, n_in - 1)
        return np.ascontiguousarray(w), np.ascontiguousarray(idx)
    rho = (1.0 / float(scale_factor)) if scale_factor is not None else float(n_in) / float(n_out)
    s = (o.astype(np.float64) + 0.5) * rho - 0.5
    if mode == "bilinear":
        s = np.maximum(s, 0.0)
        i0 = np.floor(s).astype(np.int64)
        lam = s - i0
        i0 = np.minimum(i0, n_in - 1)
        idx = np.stack([i0, np.minimum(i0 + 1, n_in - 1)], axis=1)
        return np.stack([1.0 - lam, lam], axis=1), idx
    fl = np.floor(s)
    w = _cubic_torch(s - fl)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], 0, n_in - 1)
    return w, idx


def interpolate_tables(n_in, n_out, mode, scale_factor=None, device="cuda:0"):
    """The ``AxisTables`` (forward and transposed, the layout of ``imresize_tables``) of one axis of
    ``interpolate_axis_weights`` on `device`, cached per argument tuple."""
    if mode not in INTERPOLATE_MODES:
        raise ValueError(f"interpolate: unknown mode {mode!r}; one of {INTERPOLATE_MODES}")
    key = ("interpolate", int(n_in), int(n_out), mode, None if scale_factor is None else float(scale_factor), str(device))
    hit = _cache.get(key)
    if hit is None:
        if key[1] < 1 or key[2] < 1 or (key[4] is not None and not key[4] > 0):
            raise ValueError(f"interpolate: axis of {n_in} -> {n_out} pixels at scale factor {scale_factor}")
        w64, idx = interpolate_axis_weights(key[1], key[2], mode, key[4])
        hit = _cache[key] = AxisTables(key[1], key[2], key[2] / key[1], w64, idx, device)
    return hit


def interpolate(x, size=None, scale_factor=None, mode="bilinear"):
    """``torch.nn.functional.interpolate(x, size=, scale_factor=, mode=, align_corners=False)`` without antialias, for mode
    "area", "bilinear" or "bicubic", on a floating-point ``[N, C, H, W]`` device tensor: the tables of ``interpolate_tables``
    run through ``functional.Imresize`` (dsr_imresize_f32; fp32 out, differentiable with respect to `x`).  Exactly one of
    ``size`` = (OH, OW) and ``scale_factor`` (a float or a pair; the output is ``floor(n s)`` long)."""
    if not (torch.is_tensor(x) and x.is_floating_point() and x.dim() == 4):
        raise TypeError("interpolate: a floating-point [N, C, H, W] tensor is expected")
    if mode not in INTERPOLATE_MODES:
        raise ValueError(f"interpolate: unknown mode {mode!r}; one of {INTERPOLATE_MODES}")
    if (size is None) == (scale_factor is None):
        raise ValueError("interpolate: exactly one of `size` and `scale_factor` is expected")
    h, w = int(x.shape[2]), int(x.shape[3])
    if size is not None:
        oh, ow = (interpolate_out_size(n, size=v) for n, v in zip((h, w), size))
        sh = sw = None
    else:
        sh, sw = (scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor))
        oh, ow = interpolate_out_size(h, scale_factor=sh), interpolate_out_size(w, scale_factor=sw)
    _need_gpu(x)
    return F.Imresize.apply(x, interpolate_tables(h, oh, mode, sh, x.device), interpolate_tables(w, ow, mode, sw, x.device))


def modcrop(image, scale):
    """`image` with H and W cropped (at the bottom / right) to multiples of `scale`: ``[..., H, W]`` for a floating-point
    tensor, ``[H, W, C]`` for a uint8 tensor or numpy array, or a PIL image."""
    scale = int(scale)
    if scale < 1:
        raise ValueError(f"modcrop: scale {scale}")
    if torch.is_tensor(image) and image.is_floating_point():
        h, w = image.shape[-2], image.shape[-1]
        return image[..., :h - h % scale, :w - w % scale]
    if torch.is_tensor(image) or isinstance(image, np.ndarray):
        h, w = image.shape[0], image.shape[1]
        return image[:h - h % scale, :w - w % scale]
    w, h = image.width, image.height
    return image.crop((0, 0, w - w % scale, h - h % scale))


class Imresize(torch.nn.Module):
    """``imresize`` as a module with the same arguments: no parameters, no buffers.  A drop-in for the `downsampler` of
    ``steps.DipRunner`` and the ``utils.DIP`` closures -- the forward model of a benchmark LR image."""

    def __init__(self, scale=None, size=None, kernel="bicubic", antialiasing=True):
        super().__init__()
        if (scale is None) == (size is None):
            raise ValueError("Imresize: exactly one of `scale` and `size` is expected")
        _check_kernel(kernel)
        self.scale, self.size, self.kernel, self.antialiasing = scale, size, kernel, bool(antialiasing)

    def forward(self, x):
        return imresize(x, scale=self.scale, size=self.size, kernel=self.kernel, antialiasing=self.antialiasing)

    def extra_repr(self):
        what = f"scale={self.scale}" if self.size is None else f"size={tuple(self.size)}"
        return f"{what}, kernel={self.kernel!r}, antialiasing={self.antialiasing}"
