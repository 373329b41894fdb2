"""PSNR and SSIM as metric modules on the HIP path: the two objects the reference's scripts build next to LPIPS
(torchmetrics ``PeakSignalNoiseRatio()`` and ``StructuralSimilarityIndexMeasure(data_range=1.0)``: train_GAN.py:30-31,110-111,
eval_GAN.py:30-31,47-48, DIP.py:73-74,157-158,183-184).

torchmetrics is absent here, so both restate its documented behaviour -- PARITY UNPINNED, as for ``lpips.LPIPS`` and
``evaluate.psnr``:
  PSNR  10 / ln(base) * (2 ln(range) - ln(SSE / count)); with ``dim=None`` over the whole batch (and every batch added by
        ``update``), with ``dim=(1, 2, 3)`` per image, then reduced.  ``data_range=None`` takes the range from the target as
        max(running max, target max) - min(running min, target min), the running pair starting at 0.
  SSIM  Wang, Bovik, Sheikh, Simoncelli 2004 with a Gaussian 11x11 window (sigma 1.5), K1 = 0.01, K2 = 0.03, per channel, the
        mean over every window position inside the image (torchmetrics reflect-pads by 5 and crops that border again: the same
        positions), per image; then the batch mean, sum, or the [N] values (``reduction``).

Both behave like a torchmetrics ``Metric`` with ``full_state_update=False``: ``forward`` returns the batch's value from a fresh
state and adds the batch to the running state; ``update`` / ``compute`` / ``reset`` keep that state on the device (sums, counts
and PSNR's running min / max, in float64).  Nothing here reads a device value on the host, so a call can be captured in a HIP
graph (steps.GraphedStep).

Device work (csrc/metrics.hip, include/dsr_hip.h):
  dsr_ssim_img_f32     per-image SSIM: separable row / column passes over an LDS tile, one partial per block, a one-block fold;
  dsr_ssim_bwd_f32     its input gradient for either image or both in one launch, the moments recomputed per tile;
  dsr_psnr_stats_f32   one pass: per-block squared-error sums and the target's min / max as order-preserving keys;
  dsr_psnr_finalize    per-image or whole-batch PSNR and the running-state update;
  dsr_metric_accumulate / dsr_metric_compute   the running state.
SSIM is differentiable (a loss term such as ``1 - ssim(x, y)``); PSNR is not.

``MultiScaleStructuralSimilarityIndexMeasure`` (alias ``MS_SSIM``) restates torchmetrics' module of that name in the same way
-- PARITY UNPINNED too.  Per scale s = 0 .. L-1 (L = len(betas)) the current pair of images gives, over the same window positions
as SSIM, the per-image means of ``cs = (2 cov + c2) / (var_a + var_b + c2)`` and of ``ssim = cs * (2 mu_a mu_b + c1) /
(mu_a^2 + mu_b^2 + c1)``; ``normalize='relu'`` clamps both at 0; then both images are replaced by their 2x2 mean at stride 2
(``F.avg_pool2d(x, 2)``: an odd last row or column is dropped).  With v = (cs_0, .., cs_{L-2}, ssim_{L-1}), halved to
(v + 1) / 2 under ``normalize='simple'``, the per-image value is prod_s v_s ** betas[s].  Device work:
  dsr_ssim_cs_img_f32     the two per-image means of one scale (the SSIM tile kernel with two partials per block, one fold);
  dsr_avgpool2_pair_f32   both images to half size in one launch;
  dsr_msssim_combine      normalised values, powers, product, the reduction's total and d out / d (per-scale mean), one launch;
  dsr_msssim_bwd_f32      one scale of the backward: each image carries a weight for its SSIM mean and one for its cs mean, and
                          the epilogue adds the coarser scale's gradient spread back through the pool -- L launches, coarse to fine.

``LumaPeakSignalNoiseRatio`` (``PSNR_Y``), ``LumaStructuralSimilarityIndexMeasure`` (``SSIM_Y``) and ``rgb_to_y`` are the
evaluation protocol of the published super-resolution tables (SRGAN, ESRGAN, EDSR, ...; basicsr's ``calculate_psnr`` /
``calculate_ssim`` with ``test_y_channel=True`` and MATLAB's ``rgb2ycbcr``) -- PARITY UNPINNED as well, neither is installed
here: the output is quantised to 8 bits, ``shave`` pixels are cut from each border, RGB becomes the BT.601 luma
``Y = (16 + 65.481 r + 128.553 g + 24.966 b) / 255``, and PSNR / SSIM are taken per image on that one plane, then averaged.
Device work (csrc/luma.hip), reading fp32 / fp16 / bf16 [N,3,H,W] as they are:
  dsr_luma_sse_stats       one pass over both images: per-block sums of dY^2 over the cropped region, dY formed from the
                           channel differences (exact integers / 255 when quantised), nothing of image size written;
  dsr_luma_pair            both cropped luma planes in one launch (they feed dsr_ssim_img_f32 with C = 1), optionally with the
                           same partial sums: one read of each frame for both metrics;
  dsr_rgb_to_y             one tensor's plane;
  dsr_luma_psnr_finalize   per-image 10 log10(count / SSE_n), the reduction's total and the running state.

``NaturalnessImageQualityEvaluator`` (``NIQE``) and ``niqe_features`` score an image WITHOUT a ground truth, the way the
Real-ESRGAN paper and BasicSR's ``calculate_niqe`` do -- PARITY UNPINNED again; the definition is in the class docstring and, in
float64 numpy, in tests/niqe_ref.py.  Device work (csrc/niqe.hip), float64 from the luma plane onward:
  dsr_niqe_plane           the rounded 8-bit luma, shaved and cropped to whole 96 x 96 blocks (bit-exact integer arithmetic);
  dsr_imresize_f32         its half-size copy for scale 2 (csrc/imresize.hip);
  dsr_niqe_moments         per block the MSCN image in LDS and the five sums of each of its five maps, one launch per scale;
  dsr_niqe_features        the AGGD fits: 36 features per block.
The block statistics are a few float64 torch ops on the device; the 36 x 36 pseudo-inverse is numpy's, on the host.
"""
import ctypes as C
import math
import numbers

import torch
import torch.nn as nn

from . import _lib
from ._lib import _ptr, _stream, check

_WIN = 11
_REDUCTIONS = ("elementwise_mean", "sum", "none", None)


def _check_pair(name, preds, target):
    """Both inputs 4-D tensors of one shape, at least 11 x 11, on the device.  Returns (N, C, H, W)."""
    for t in (preds, target):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: expected two [N, C, H, W] tensors, got "
                             f"{tuple(preds.shape) if torch.is_tensor(preds) else type(preds).__name__} and "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
    if preds.shape != target.shape:
        raise ValueError(f"{name}: the two inputs must have one shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    n, c, h, w = preds.shape
    if n < 1 or c < 1:
        raise ValueError(f"{name}: empty batch {tuple(preds.shape)}")
    if h < _WIN or w < _WIN:
        raise ValueError(f"{name}: images of {h}x{w} are smaller than 11x11")
    if not (preds.is_floating_point() and target.is_floating_point()):
        raise ValueError(f"{name}: expected floating-point inputs, got {preds.dtype} and {target.dtype}")
    if not (preds.is_cuda and target.is_cuda):
        raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                           "there is no CPU implementation of this path")
    return n, c, h, w


def _f32(t):
    """fp32 contiguous view of t, detached (fp16 / bf16 / fp64 inputs are computed in fp32)."""
    return t.detach().contiguous().float()


def _positive_float(name, what, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (float(v) > 0 and math.isfinite(float(v))):
        raise ValueError(f"{name}: {what} must be a positive finite number, got {v!r}")
    return float(v)


def _check_reduction(name, reduction):
    if reduction not in _REDUCTIONS:
        raise ValueError(f"{name}: reduction must be one of 'elementwise_mean', 'sum', 'none' or None, got {reduction!r}")
    return "none" if reduction is None else reduction


class _RunningState:
    """float64 [4] device state (see dsr_psnr_finalize / dsr_metric_accumulate) and, for reduction 'none', the per-image
    values of every update.  ``updated`` is a host flag set by the calls themselves: no device read."""

    def __init__(self):
        self.buf = None
        self.values = []
        self.updated = False

    def get(self, dev):
        if self.buf is None or self.buf.device != dev:
            self.buf = torch.zeros(4, dtype=torch.float64, device=dev)     # PSNR's running min / max start at 0
        return self.buf


class PeakSignalNoiseRatio(nn.Module):
    """torchmetrics ``PeakSignalNoiseRatio(data_range, base, reduction, dim)`` on the HIP path (not differentiable).

    ``dim``: None (one value over everything seen) or (1, 2, 3) (per image, then ``reduction``: 'elementwise_mean', 'sum',
    'none' / None; needs ``data_range``).  ``data_range``: a positive number, or None to infer it from the targets as above.
    A tuple ``data_range`` (torchmetrics clamps the inputs to it) and other ``dim``s are not built here.  Inputs are [N,C,H,W]
    of one shape and at least 11 x 11, like SSIM's (the two modules take the same batches at every call site)."""

    def __init__(self, data_range=None, base=10.0, reduction="elementwise_mean", dim=None):
        super().__init__()
        if isinstance(data_range, (tuple, list)):
            raise NotImplementedError("PeakSignalNoiseRatio: data_range as a (min, max) tuple (clamping the inputs) is not "
                                      "built here; pass a number or None")
        if dim is not None:
            d = (dim,) if isinstance(dim, int) else tuple(dim)
            if tuple(sorted(d)) != (1, 2, 3):
                raise NotImplementedError(f"PeakSignalNoiseRatio: dim={dim!r} is not built here; only None and (1, 2, 3) are")
            if data_range is None:
                raise ValueError("PeakSignalNoiseRatio: the `data_range` must be given when `dim` is not None")
        self.dim = None if dim is None else (1, 2, 3)
        self.data_range = None if data_range is None else _positive_float("PeakSignalNoiseRatio", "data_range", data_range)
        b = _positive_float("PeakSignalNoiseRatio", "base", base)
        if b == 1.0:
            raise ValueError("PeakSignalNoiseRatio: base must not be 1")
        self.base = b
        self.log_scale = 10.0 / math.log(b)
        self.reduction = _check_reduction("PeakSignalNoiseRatio", reduction)
        self._st = _RunningState()

    # ---- running state
    def reset(self):
        self._st = _RunningState()

    def update(self, preds, target):
        self._batch(preds, target)

    def forward(self, preds, target):
        return self._batch(preds, target)

    def compute(self):
        st = self._st
        if not st.updated:
            raise RuntimeError("PeakSignalNoiseRatio.compute() called before update()")
        if self.dim is not None and self.reduction == "none":
            return torch.cat(st.values)
        out = torch.empty(1, dtype=torch.float32, device=st.buf.device)
        if self.dim is None:
            mode = 2
        else:
            mode = 1 if self.reduction == "elementwise_mean" else 0
        check(_lib.lib().dsr_metric_compute(_ptr(st.buf), mode, int(self.data_range is None), self._range(), self.log_scale,
                                            _ptr(out), _stream()))
        return out.reshape(())

    # ---- the device path
    def _range(self):
        return 1.0 if self.data_range is None else self.data_range       # (ignored when inferred)

    def _batch(self, preds, target):
        """The batch's value from a fresh state; the batch is added to the running state."""
        n, c, h, w = _check_pair("PeakSignalNoiseRatio", preds, target)
        e = c * h * w
        lib = _lib.lib()
        st = _stream()
        dev = preds.device
        p, t = _f32(preds), _f32(target)
        blocks = lib.dsr_psnr_blocks(n, e)
        if blocks <= 0:
            raise RuntimeError(f"PeakSignalNoiseRatio: {n} images of {e} elements are too many for one launch")
        sse = torch.empty(blocks, dtype=torch.float32, device=dev)
        keys = torch.empty(2 * blocks, dtype=torch.int32, device=dev)
        check(lib.dsr_psnr_stats_f32(_ptr(p), _ptr(t), n, e, _ptr(sse), _ptr(keys), st))
        state = self._st.get(dev)
        if self.dim is None:
            val = torch.empty(1, dtype=torch.float32, device=dev)
            check(lib.dsr_psnr_finalize(_ptr(sse), _ptr(keys), n, e, int(self.data_range is None), self._range(),
                                        self.log_scale, None, _ptr(val), 1.0, _ptr(state), st))
            out = val.reshape(())
        else:
            per = torch.empty(n, dtype=torch.float32, device=dev)
            val = None if self.reduction == "none" else torch.empty(1, dtype=torch.float32, device=dev)
            scale = 1.0 / n if self.reduction == "elementwise_mean" else 1.0
            check(lib.dsr_psnr_finalize(_ptr(sse), _ptr(keys), n, e, 0, self.data_range, self.log_scale, _ptr(per), _ptr(val),
                                        scale, _ptr(state), st))
            if self.reduction == "none":
                self._st.values.append(per.clone())
                out = per
            else:
                out = val.reshape(())
        self._st.updated = True
        return out


class _PerImageMetric(nn.Module):
    """The running state, reduction and upstream gradient shared by the metrics that fold one fp32 value per image."""

    def _init_state(self, reduction):
        self.reduction = _check_reduction(type(self).__name__, reduction)
        self._st = _RunningState()

    def reset(self):
        self._st = _RunningState()

    def compute(self):
        st = self._st
        if not st.updated:
            raise RuntimeError(f"{type(self).__name__}.compute() called before update()")
        if self.reduction == "none":
            return torch.cat(st.values)
        out = torch.empty(1, dtype=torch.float32, device=st.buf.device)
        mode = 1 if self.reduction == "elementwise_mean" else 0
        check(_lib.lib().dsr_metric_compute(_ptr(st.buf), mode, 0, 1.0, 1.0, _ptr(out), _stream()))
        return out.reshape(())

    def _total_scale(self, n):
        return 1.0 / n if self.reduction == "elementwise_mean" else 1.0

    def _accumulate(self, per):
        st = self._st
        check(_lib.lib().dsr_metric_accumulate(_ptr(per), per.shape[0], _ptr(st.get(per.device)), _stream()))
        if self.reduction == "none":
            st.values.append(per.clone())
        st.updated = True

    def _upstream(self, gper, gtot, n, dev):
        """fp32 [n]: d loss / d per_image[i] = gper[i] + total_scale * gtot, formed on the device."""
        lib = _lib.lib()
        g = None
        if gtot is not None:
            ones = torch.ones(n, dtype=torch.float32, device=dev)
            g = torch.empty(n, dtype=torch.float32, device=dev)
            check(lib.dsr_pw_axpby_f32(_ptr(ones), None, self._total_scale(n), 0.0, _ptr(gtot.contiguous().float()), _ptr(g), n,
                                       _stream()))
        if gper is not None:
            gper = gper.contiguous().float()
            if g is None:
                return gper
            both = torch.empty(n, dtype=torch.float32, device=dev)
            check(lib.dsr_pw_axpby_f32(_ptr(gper), _ptr(g), 1.0, 1.0, None, _ptr(both), n, _stream()))
            return both
        return g


def _check_window(name, gaussian_kernel, sigma, kernel_size):
    """The one window both SSIM modules are built for: Gaussian, 11 x 11, sigma 1.5."""
    if not gaussian_kernel:
        raise NotImplementedError(f"{name}: gaussian_kernel=False (a uniform window) is not built here")
    sig = tuple(sigma) if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    if len(sig) != 2 or any(isinstance(s, bool) or not isinstance(s, numbers.Real) or float(s) != 1.5 for s in sig):
        raise NotImplementedError(f"{name}: sigma={sigma!r} is not built here; only 1.5 is")
    ks = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    if len(ks) != 2 or any(isinstance(k, bool) or k != _WIN for k in ks):
        raise NotImplementedError(f"{name}: kernel_size={kernel_size!r} is not built here; only 11 is")


def _check_constants(name, data_range, k1, k2):
    """(data_range, k1, k2, c1, c2) with c = (k * data_range)^2 inside the fp32 range."""
    if data_range is None:
        raise NotImplementedError(f"{name}: data_range=None (inferred from the inputs) is not built here; pass a number")
    if isinstance(data_range, (tuple, list)):
        raise NotImplementedError(f"{name}: data_range as a (min, max) tuple (clamping the inputs) is not built here")
    data_range = _positive_float(name, "data_range", data_range)
    k1 = _positive_float(name, "k1", k1)
    k2 = _positive_float(name, "k2", k2)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    if not (0 < float(C.c_float(c1).value) < math.inf and 0 < float(C.c_float(c2).value) < math.inf):
        raise ValueError(f"{name}: (k * data_range)^2 leaves the fp32 range")
    return data_range, k1, k2, c1, c2


def _ssim_img(name, a, b, c1, c2, scale, want_total=True):
    """(per_image [N], total [1] = scale * their sum, or None): dsr_ssim_img_f32 on two fp32 [N,C,H,W] tensors of one shape,
    each side at least the window's.  The one SSIM forward launch: the SSIM modules and ``evaluate.ssim`` all come here."""
    n, c, h, w = a.shape
    lib = _lib.lib()
    blocks = lib.dsr_ssim_img_blocks(n, c, h, w)
    if blocks <= 0:
        raise RuntimeError(f"{name}: {tuple(a.shape)} needs too many window tiles")
    dev = a.device
    partial = torch.empty(blocks, dtype=torch.float32, device=dev)
    per = torch.empty(n, dtype=torch.float32, device=dev)
    tot = torch.empty(1, dtype=torch.float32, device=dev) if want_total else None
    check(lib.dsr_ssim_img_f32(_ptr(a), _ptr(b), n, c, h, w, c1, c2, _ptr(partial), _ptr(per), _ptr(tot), scale, 0, _stream()))
    return per, tot


class StructuralSimilarityIndexMeasure(_PerImageMetric):
    """torchmetrics ``StructuralSimilarityIndexMeasure`` on the HIP path, for what the reference uses: the Gaussian 11x11 window
    with sigma 1.5 and a positive ``data_range`` (the reference passes 1.0).  ``reduction``: 'elementwise_mean' (0-dim),
    'sum' (0-dim) or 'none' / None ([N], one value per image).

    ``forward`` is differentiable with respect to either input or both when grad mode is on and an input requires a gradient:
    ``1 - ssim(x, y)`` is a loss term.  ``update`` never is."""

    def __init__(self, gaussian_kernel=True, sigma=1.5, kernel_size=11, reduction="elementwise_mean", data_range=1.0,
                 k1=0.01, k2=0.03, return_full_image=False, return_contrast_sensitivity=False):
        super().__init__()
        name = "StructuralSimilarityIndexMeasure"
        _check_window(name, gaussian_kernel, sigma, kernel_size)
        if return_full_image:
            raise NotImplementedError(f"{name}: return_full_image=True is not built here")
        if return_contrast_sensitivity:
            raise NotImplementedError(f"{name}: return_contrast_sensitivity=True is not built here")
        self.data_range, self.k1, self.k2, self.c1, self.c2 = _check_constants(name, data_range, k1, k2)
        self._init_state(reduction)

    def update(self, preds, target):
        _check_pair("StructuralSimilarityIndexMeasure", preds, target)
        per, _ = self._run(preds, target)
        self._accumulate(per)

    def forward(self, preds, target):
        _check_pair("StructuralSimilarityIndexMeasure", preds, target)
        if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
            per, tot = _SSIMFunction.apply(self, preds, target)
        else:
            per, tot = self._run(preds, target)
        self._accumulate(per.detach())
        return per if self.reduction == "none" else tot.reshape(())

    # ---- the device path
    def _run(self, preds, target, a=None, b=None):
        """(per_image [N], total [1] = the reduction's scale * sum) of fp32 copies a, b of the inputs."""
        a = _f32(preds) if a is None else a
        b = _f32(target) if b is None else b
        return _ssim_img("StructuralSimilarityIndexMeasure", a, b, self.c1, self.c2, self._total_scale(a.shape[0]))


class _SSIMFunction(torch.autograd.Function):
    """(per_image [N], total [1]) of StructuralSimilarityIndexMeasure._run, with dsr_ssim_bwd_f32 as the backward."""

    @staticmethod
    def forward(ctx, mod, preds, target):
        a, b = _f32(preds), _f32(target)
        per, tot = mod._run(preds, target, a, b)
        ctx.mod, ctx.a, ctx.b = mod, a, b
        ctx.dtypes = (preds.dtype, target.dtype)
        ctx.set_materialize_grads(False)
        return per, tot

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, gtot):
        want1, want2 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want1 or want2) or (gper is None and gtot is None):
            return None, None, None
        mod, a, b = ctx.mod, ctx.a, ctx.b
        n, c, h, w = a.shape
        g = mod._upstream(gper, gtot, n, a.device)
        g1 = torch.empty_like(a) if want1 else None
        g2 = torch.empty_like(b) if want2 else None
        check(_lib.lib().dsr_ssim_bwd_f32(_ptr(a), _ptr(b), n, c, h, w, mod.c1, mod.c2, _ptr(g), _ptr(g1), _ptr(g2), _stream()))
        out = [o if o is None or o.dtype == dt else o.to(dt) for o, dt in zip((g1, g2), ctx.dtypes)]
        return None, out[0], out[1]


_DEFAULT_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_MAX_SCALES = 8
_NORMALIZE = {None: 0, "relu": 1, "simple": 2}


class MultiScaleStructuralSimilarityIndexMeasure(_PerImageMetric):
    """torchmetrics ``MultiScaleStructuralSimilarityIndexMeasure`` on the HIP path (restated, PARITY UNPINNED: see the module
    docstring for the definition), for the Gaussian 11x11 window with sigma 1.5 and a positive ``data_range``.

    ``betas``: 1 to 8 positive finite exponents, one per scale.  Inputs are [N, C, H, W] with H, W >= 11 * 2^(len(betas) - 1)
    (176 for the default five scales, the bound torchmetrics applies).  ``normalize``: 'relu', 'simple' or None.  ``reduction``
    as for SSIM.  ``last_scales`` holds the [L, N] normalised per-scale values of the latest call (device, fp32).

    ``forward`` is differentiable like SSIM's; ``alpha * (1 - ms_ssim(x, y)) + (1 - alpha) * L1`` is steps.gen_msssim_step.
    The one deliberate difference from torch autograd of the same formula: where 'relu' clamps a per-scale value to 0 the
    image's value is 0 and its gradient is defined as 0 (autograd gives NaN there, 0 * inf).  With ``normalize=None`` a negative
    per-scale mean is the caller's risk, as in torchmetrics: NaN propagates."""

    def __init__(self, gaussian_kernel=True, kernel_size=11, sigma=1.5, reduction="elementwise_mean", data_range=1.0,
                 k1=0.01, k2=0.03, betas=_DEFAULT_BETAS, normalize="relu"):
        super().__init__()
        name = "MultiScaleStructuralSimilarityIndexMeasure"
        _check_window(name, gaussian_kernel, sigma, kernel_size)
        self.data_range, self.k1, self.k2, self.c1, self.c2 = _check_constants(name, data_range, k1, k2)
        if not isinstance(betas, (tuple, list)) or not 1 <= len(betas) <= _MAX_SCALES:
            raise ValueError(f"{name}: betas must be a tuple or list of 1 to {_MAX_SCALES} numbers, got {betas!r}")
        self.betas = tuple(_positive_float(name, "each of betas", b) for b in betas)
        if any(not (0 < float(C.c_float(b).value) < math.inf) for b in self.betas):
            raise ValueError(f"{name}: betas leave the fp32 range: {betas!r}")
        if isinstance(normalize, bool) or normalize not in _NORMALIZE:
            raise ValueError(f"{name}: normalize must be 'relu', 'simple' or None, got {normalize!r}")
        self.normalize = normalize
        self.min_size = _WIN << (len(self.betas) - 1)
        self.last_scales = None
        self._init_state(reduction)

    def update(self, preds, target):
        self._check(preds, target)
        per, _ = self._run(_f32(preds), _f32(target))
        self._accumulate(per)

    def forward(self, preds, target):
        self._check(preds, target)
        if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
            per, tot = _MSSSIMFunction.apply(self, preds, target)
        else:
            per, tot = self._run(_f32(preds), _f32(target))
        self._accumulate(per.detach())
        return per if self.reduction == "none" else tot.reshape(())

    # ---- the device path
    def _check(self, preds, target):
        """As _check_pair, with the pyramid's size rule in front of the device check: every refusal precedes any launch."""
        name = "MultiScaleStructuralSimilarityIndexMeasure"
        if torch.is_tensor(preds) and torch.is_tensor(target) and preds.dim() == 4 and preds.shape == target.shape:
            h, w = preds.shape[2:]
            if min(h, w) >= _WIN and min(h, w) < self.min_size:
                raise ValueError(f"{name}: images of {h}x{w} are smaller than {self.min_size}x{self.min_size}, which "
                                 f"{len(self.betas)} scales need (11 * 2^(scales - 1))")
        return _check_pair(name, preds, target)

    def _levels(self, shape):
        n, c, h, w = shape
        return [(h >> s, w >> s) for s in range(len(self.betas))]

    def _run(self, a, b, keep=False):
        """(per_image [N], total [1]) of the fp32 contiguous pair a, b; with `keep` also what the backward needs: the pooled
        levels of both images (lists of [N, C, h, w] views, level 0 = a, b) and the [L, N] factors d per_image / d scale mean."""
        n, c, h, w = a.shape
        L = len(self.betas)
        lib = _lib.lib()
        st = _stream()
        dev = a.device
        blocks = lib.dsr_ssim_cs_img_blocks(n, c, h, w)
        if blocks <= 0:
            raise RuntimeError(f"MultiScaleStructuralSimilarityIndexMeasure: {tuple(a.shape)} needs too many window tiles")
        levels = self._levels(a.shape)
        pyr = int(lib.dsr_msssim_pyramid_floats(n, c, h, w, L))
        pa = torch.empty(max(pyr, 1), dtype=torch.float32, device=dev)
        pb = torch.empty(max(pyr, 1), dtype=torch.float32, device=dev)
        la, lb, off = [a], [b], 0
        for hs, ws in levels[1:]:
            cnt = n * c * hs * ws
            la.append(pa[off:off + cnt].view(n, c, hs, ws))
            lb.append(pb[off:off + cnt].view(n, c, hs, ws))
            off += cnt
        partial = torch.empty(2 * blocks, dtype=torch.float32, device=dev)       # scale 0 has the most blocks
        raw = torch.empty(L, n, dtype=torch.float32, device=dev)
        for s, (hs, ws) in enumerate(levels):
            last = s == L - 1
            check(lib.dsr_ssim_cs_img_f32(_ptr(la[s]), _ptr(lb[s]), n, c, hs, ws, self.c1, self.c2, _ptr(partial),
                                          _ptr(raw[s]) if last else None, None if last else _ptr(raw[s]), st))
            if not last:
                check(lib.dsr_avgpool2_pair_f32(_ptr(la[s]), _ptr(lb[s]), _ptr(la[s + 1]), _ptr(lb[s + 1]), n * c, hs, ws, st))
        vals = torch.empty(L, n, dtype=torch.float32, device=dev)
        per = torch.empty(n, dtype=torch.float32, device=dev)
        tot = torch.empty(1, dtype=torch.float32, device=dev)
        factors = torch.empty(L, n, dtype=torch.float32, device=dev) if keep else None
        check(lib.dsr_msssim_combine(_ptr(raw), n, L, (C.c_float * L)(*self.betas), _NORMALIZE[self.normalize], _ptr(vals), _ptr(per), _ptr(tot),
                                     self._total_scale(n), _ptr(factors), st))
        self.last_scales = vals
        if keep:
            return per, tot, la, lb, factors
        return per, tot


class _MSSSIMFunction(torch.autograd.Function):
    """(per_image [N], total [1]) of MultiScaleStructuralSimilarityIndexMeasure._run; the backward is one dsr_msssim_bwd_f32
    per scale from the coarsest to the finest, each adding the coarser gradient through the pool in its epilogue."""

    @staticmethod
    def forward(ctx, mod, preds, target):
        a, b = _f32(preds), _f32(target)
        per, tot, la, lb, factors = mod._run(a, b, keep=True)
        ctx.mod, ctx.la, ctx.lb, ctx.factors = mod, la, lb, factors
        ctx.dtypes = (preds.dtype, target.dtype)
        ctx.set_materialize_grads(False)
        return per, tot

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, gtot):
        want1, want2 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want1 or want2) or (gper is None and gtot is None):
            return None, None, None
        mod, la, lb, factors = ctx.mod, ctx.la, ctx.lb, ctx.factors
        n, c = la[0].shape[:2]
        L = len(la)
        lib = _lib.lib()
        st = _stream()
        g = mod._upstream(gper, gtot, n, la[0].device)
        g1 = g2 = None
        for s in range(L - 1, -1, -1):
            hs, ws = la[s].shape[2:]
            last = s == L - 1
            n1 = torch.empty_like(la[s]) if want1 else None
            n2 = torch.empty_like(lb[s]) if want2 else None
            check(lib.dsr_msssim_bwd_f32(_ptr(la[s]), _ptr(lb[s]), n, c, hs, ws, mod.c1, mod.c2, _ptr(g),
                                         _ptr(factors[s]) if last else None, None if last else _ptr(factors[s]),
                                         _ptr(g1), _ptr(g2), _ptr(n1), _ptr(n2), st))
            g1, g2 = n1, n2
        out = [o if o is None or o.dtype == dt else o.to(dt) for o, dt in zip((g1, g2), ctx.dtypes)]
        return None, out[0], out[1]


# ============================================================================= Y-channel PSNR / SSIM with a border shave
_LUMA_DTYPES = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.F32}


def _check_shave(name, shave):
    if isinstance(shave, bool) or not isinstance(shave, numbers.Integral) or shave < 0:
        raise ValueError(f"{name}: shave must be a non-negative integer, got {shave!r}")
    return int(shave)


def _check_rgb(name, x, shave, min_side):
    """x: a floating-point [N, 3, H, W] tensor whose shaved region is at least min_side x min_side, on the device.
    Returns (N, H, W)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{name}: expected [N, 3, H, W] tensors, got "
                         f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError(f"{name}: the luma is defined for RGB, got {c} channels in {tuple(x.shape)}")
    if n < 1:
        raise ValueError(f"{name}: empty batch {tuple(x.shape)}")
    if not x.is_floating_point():
        raise ValueError(f"{name}: expected floating-point inputs, got {x.dtype}")
    if h - 2 * shave < min_side or w - 2 * shave < min_side:
        raise ValueError(f"{name}: shave={shave} leaves {max(h - 2 * shave, 0)}x{max(w - 2 * shave, 0)} of a {h}x{w} image; "
                         f"at least {min_side}x{min_side} is needed")
    return n, h, w


def _check_rgb_pair(name, preds, target, shave, min_side):
    for t in (preds, target):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: expected two [N, 3, H, W] tensors, got "
                             f"{tuple(preds.shape) if torch.is_tensor(preds) else type(preds).__name__} and "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
    if preds.shape != target.shape:
        raise ValueError(f"{name}: the two inputs must have one shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    n, h, w = _check_rgb(name, preds, shave, min_side)
    _check_rgb(name, target, shave, min_side)
    if not (preds.is_cuda and target.is_cuda):
        raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                           "there is no CPU implementation of this path")
    return n, h, w


def _luma_in(t):
    """(dtype code, tensor) as the luma kernels read it: fp32 / fp16 / bf16 as they are, any other float type as fp32."""
    t = t.detach()
    if t.dtype not in _LUMA_DTYPES:
        t = t.float()
    return _LUMA_DTYPES[t.dtype], t.contiguous()


def rgb_to_y(x, shave=0, quantize=False):
    """fp32 [N, 1, H - 2 shave, W - 2 shave]: the BT.601 luma ``(16 + 65.481 r + 128.553 g + 24.966 b) / 255`` of MATLAB's
    ``rgb2ycbcr`` in unit scale (white 235/255, black 16/255) of an [N, 3, H, W] tensor in fp32, fp16 or bf16, with ``shave``
    pixels cut from each border; ``quantize`` first rounds each channel to its 8-bit code, ``round(clamp(x, 0, 1) * 255) /
    255``.  Not differentiable.  PARITY UNPINNED (see the module docstring)."""
    shave = _check_shave("rgb_to_y", shave)
    n, h, w = _check_rgb("rgb_to_y", x, shave, 1)
    if not x.is_cuda:
        raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                           "there is no CPU implementation of this path")
    dt, xx = _luma_in(x)
    y = torch.empty(n, 1, h - 2 * shave, w - 2 * shave, dtype=torch.float32, device=x.device)
    check(_lib.lib().dsr_rgb_to_y(dt, _ptr(xx), n, 3, h, w, shave, int(bool(quantize)), _ptr(y), _stream()))
    return y


def _luma_stats(name, preds, target, shave, quantize, planes):
    """One pass over both images: (partial sums of dY^2, the two cropped luma planes or None)."""
    n, _, h, w = preds.shape
    lib = _lib.lib()
    dev = preds.device
    blocks = lib.dsr_luma_blocks(n, h, w, shave)
    if blocks <= 0:
        raise RuntimeError(f"{name}: {tuple(preds.shape)} is too large for one launch")
    dp, p = _luma_in(preds)
    dt, t = _luma_in(target)
    sse = torch.empty(blocks, dtype=torch.float32, device=dev)
    if not planes:
        check(lib.dsr_luma_sse_stats(dp, _ptr(p), dt, _ptr(t), n, 3, h, w, shave, int(quantize), _ptr(sse), _stream()))
        return sse, None, None
    yp = torch.empty(n, 1, h - 2 * shave, w - 2 * shave, dtype=torch.float32, device=dev)
    yt = torch.empty_like(yp)
    check(lib.dsr_luma_pair(dp, _ptr(p), dt, _ptr(t), n, 3, h, w, shave, int(quantize), _ptr(yp), _ptr(yt),
                            _ptr(sse) if planes == "both" else None, _stream()))
    return (sse if planes == "both" else None), yp, yt


def _luma_psnr(sse, n, h, w, shave, scale, state, dev, want_total=True):
    """(per_image [N], total [1] or None) from the partial sums; `state` (float64 [4] or None) takes the batch."""
    per = torch.empty(n, dtype=torch.float32, device=dev)
    tot = torch.empty(1, dtype=torch.float32, device=dev) if want_total else None
    check(_lib.lib().dsr_luma_psnr_finalize(_ptr(sse), n, h, w, shave, _ptr(per), _ptr(tot), scale, _ptr(state), _stream()))
    return per, tot


_SSIM_C1, _SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def _luma_ssim(yp, yt, scale, want_total=True):
    """(per_image [N], total [1] or None) of the two luma planes (C = 1, data_range 1)."""
    return _ssim_img("LumaStructuralSimilarityIndexMeasure", yp, yt, _SSIM_C1, _SSIM_C2, scale, want_total)


def luma_psnr_ssim(preds, target, shave=0, quantize=True, with_ssim=True):
    """(PSNR-Y [N], SSIM-Y [N] or None) per image, fp32 on the device, from ONE read of the two frames: the luma-pair launch
    writes both cropped planes and the squared-error partials, then the PSNR fold and the SSIM tile + fold launches (4 launches;
    2 without SSIM).  Nothing is read on the host.  The loop of ``evaluate.evaluate_generator(y_channel=True)``."""
    name = "luma_psnr_ssim"
    shave = _check_shave(name, shave)
    n, h, w = _check_rgb_pair(name, preds, target, shave, _WIN if with_ssim else 1)
    sse, yp, yt = _luma_stats(name, preds, target, shave, bool(quantize), "both" if with_ssim else None)
    psnr, _ = _luma_psnr(sse, n, h, w, shave, 1.0, None, preds.device, want_total=False)
    if not with_ssim:
        return psnr, None
    ssim, _ = _luma_ssim(yp, yt, 1.0, want_total=False)
    return psnr, ssim


class _LumaMetric(_PerImageMetric):
    """Options, input checks and the forward / update pair shared by the two Y-channel metrics."""
    _min_side = 1

    def __init__(self, shave=0, quantize=True, reduction="elementwise_mean"):
        super().__init__()
        self.shave = _check_shave(type(self).__name__, shave)
        self.quantize = bool(quantize)
        self._init_state(reduction)

    def update(self, preds, target):
        self._batch(preds, target)

    def forward(self, preds, target):
        per, tot = self._batch(preds, target)
        return per if self.reduction == "none" else tot.reshape(())

    def _check(self, preds, target):
        return _check_rgb_pair(type(self).__name__, preds, target, self.shave, self._min_side)


class LumaPeakSignalNoiseRatio(_LumaMetric):
    """PSNR on the luma plane, the way super-resolution tables report it (basicsr ``calculate_psnr(crop_border=shave,
    test_y_channel=True)`` on the 8-bit output) -- PARITY UNPINNED: basicsr and MATLAB are not installed here, this restates
    their documented behaviour.  Per image, ``10 log10(1 / mean(dY^2))`` over rows and columns ``[shave, size - shave)`` with
    ``dY = (65.481 dr + 128.553 dg + 24.966 db) / 255`` and ``d. = q(preds.) - q(target.)``, ``q`` = the 8-bit quantisation
    ``round(clamp(x, 0, 1) * 255) / 255`` when ``quantize`` (default) else the identity; ``+inf`` for identical images.

    Reduced per image first (the SR convention, not torchmetrics' pooled batch MSE), then ``reduction``: 'elementwise_mean'
    (0-dim), 'sum' (0-dim) or 'none' / None ([N]).  ``forward`` / ``update`` / ``compute`` / ``reset`` and the float64 device
    state are those of the other per-image metrics here; inputs are [N, 3, H, W] in fp32, fp16 or bf16 (read as they are).
    Nothing is read on the host, so a call can be captured in a HIP graph.  Not differentiable."""

    def _batch(self, preds, target):
        n, h, w = self._check(preds, target)
        sse, _, _ = _luma_stats(type(self).__name__, preds, target, self.shave, self.quantize, None)
        st = self._st
        per, tot = _luma_psnr(sse, n, h, w, self.shave, self._total_scale(n), st.get(preds.device), preds.device)
        if self.reduction == "none":
            st.values.append(per.clone())
        st.updated = True
        return per, tot


class LumaStructuralSimilarityIndexMeasure(_LumaMetric):
    """SSIM on the luma plane, the way super-resolution tables report it (basicsr ``calculate_ssim(crop_border=shave,
    test_y_channel=True)``) -- PARITY UNPINNED: basicsr and MATLAB are not installed here, this restates their documented
    behaviour.  Both images become ``Y = (16 + 65.481 r + 128.553 g + 24.966 b) / 255`` of their 8-bit quantisation (when
    ``quantize``, the default) over rows and columns ``[shave, size - shave)``; the per-image value is the SSIM of
    ``StructuralSimilarityIndexMeasure`` (Gaussian 11x11, sigma 1.5, K1 0.01, K2 0.03, data_range 1) of that one plane, which
    must be at least 11x11.  ``reduction``, the running state, dtypes and graph capture as for ``LumaPeakSignalNoiseRatio``.
    Not differentiable."""
    _min_side = _WIN

    def _batch(self, preds, target):
        self._check(preds, target)
        _, yp, yt = _luma_stats(type(self).__name__, preds, target, self.shave, self.quantize, "planes")
        per, tot = _luma_ssim(yp, yt, self._total_scale(preds.shape[0]))
        self._accumulate(per)
        return per, tot


PSNR = PeakSignalNoiseRatio
SSIM = StructuralSimilarityIndexMeasure
MS_SSIM = MultiScaleStructuralSimilarityIndexMeasure
PSNR_Y = LumaPeakSignalNoiseRatio
SSIM_Y = LumaStructuralSimilarityIndexMeasure


# ============================================================================= NIQE: the no-reference score of blind SR
_NIQE_BLOCK = 96
_NIQE_FEATS = 36
_NIQE_GRID = 9801                         # np.arange(0.2, 10.001, 0.001)
_NIQE_KEYS = (("mu_pris_param", (1, 36)), ("cov_pris_param", (36, 36)), ("gaussian_window", (7, 7)))
_niqe_cache = {}
_niqe_warned = False


def niqe_gaussian_window():
    """float64 numpy [7, 7]: the published window, MATLAB's ``fspecial('gaussian', 7, 7 / 6)``."""
    import numpy as np
    r = np.arange(7, dtype=np.float64) - 3.0
    g = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def niqe_gamma_tables():
    """float64 numpy [3, 9801] over alpha = arange(0.2, 10.001, 0.001): Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)), sqrt(Gamma(1/a) /
    Gamma(3/a)) and Gamma(2/a) / Gamma(1/a), from ``math.gamma`` (no scipy in the product).  Built once."""
    hit = _niqe_cache.get("tables")
    if hit is None:
        import numpy as np
        grid = np.arange(0.2, 10.001, 0.001)
        g1 = np.array([math.gamma(1.0 / a) for a in grid])
        g2 = np.array([math.gamma(2.0 / a) for a in grid])
        g3 = np.array([math.gamma(3.0 / a) for a in grid])
        hit = np.stack([g2 * g2 / (g1 * g3), np.sqrt(g1 / g3), g2 / g1])
        if hit.shape != (3, _NIQE_GRID) or not (np.diff(hit[0]) > 0).all():
            raise RuntimeError("niqe: the Gamma ratio table is not strictly increasing over the alpha grid")
        _niqe_cache["tables"] = hit
    return hit


def _niqe_device_tables(dev):
    key = ("tables", str(dev))
    hit = _niqe_cache.get(key)
    if hit is None:
        hit = _niqe_cache[key] = torch.from_numpy(niqe_gamma_tables()).to(dev).contiguous()
    return hit


def load_niqe_params(params):
    """(mu [1, 36], cov [36, 36], window [7, 7]) as float64 numpy arrays from a path to a local ``.npz`` with the keys
    ``mu_pris_param``, ``cov_pris_param`` and ``gaussian_window`` (BasicSR's ``niqe_pris_params.npz`` as it is) or from a
    ``(mu, cov, window)`` tuple.  A missing key or a wrong shape is named in the error."""
    import numpy as np
    if isinstance(params, (tuple, list)):
        if len(params) != 3:
            raise ValueError(f"niqe params: expected (mu, cov, window), got {len(params)} items")
        given = dict(zip((k for k, _ in _NIQE_KEYS), params))
    else:
        with np.load(params, allow_pickle=False) as f:
            missing = [k for k, _ in _NIQE_KEYS if k not in f.files]
            if missing:
                raise KeyError(f"niqe params: {params!r} has no {missing[0]!r} (keys: {sorted(f.files)})")
            given = {k: f[k] for k, _ in _NIQE_KEYS}
    out = []
    for key, shape in _NIQE_KEYS:
        a = given[key]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if key == "mu_pris_param" and a.shape == (36,):
            a = a.reshape(1, 36)
        if a.shape != shape:
            raise ValueError(f"niqe params: {key} has shape {tuple(a.shape)}, expected {shape}")
        if not np.issubdtype(a.dtype, np.number) or not np.isfinite(a.astype(np.float64)).all():
            raise ValueError(f"niqe params: {key} holds values that are not finite numbers")
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    return tuple(out)


def _niqe_check(name, x, shave):
    """(N, H, W, hc, wc) of a floating-point [N, 3, H, W] tensor that leaves two 96 x 96 blocks; the device check comes last."""
    n, h, w = _check_rgb(name, x, shave, 1)
    nby, nbx = (h - 2 * shave) // _NIQE_BLOCK, (w - 2 * shave) // _NIQE_BLOCK
    if nby * nbx < 2:
        raise ValueError(f"{name}: shave={shave} leaves {h - 2 * shave}x{w - 2 * shave} of a {h}x{w} image; NIQE needs at least "
                         f"two 96x96 blocks")
    if n * nby * nbx * _NIQE_BLOCK * _NIQE_BLOCK >= 1 << 31:
        raise ValueError(f"{name}: {tuple(x.shape)} has more than 2^31 pixels; score it in smaller batches")
    if not x.is_cuda:
        raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                           "there is no CPU implementation of this path")
    return n, h, w, nby * _NIQE_BLOCK, nbx * _NIQE_BLOCK


def _niqe_window(window, dev):
    """The device fp64 [49] window: None = the published Gaussian (cached per device), else a [7, 7] array or tensor."""
    if window is None:
        key = ("window", str(dev))
        hit = _niqe_cache.get(key)
        if hit is None:
            hit = _niqe_cache[key] = torch.from_numpy(niqe_gaussian_window()).to(dev).reshape(49).contiguous()
        return hit
    w = window if torch.is_tensor(window) else torch.as_tensor(window)
    if tuple(w.shape) != (7, 7):
        raise ValueError(f"niqe: the window has shape {tuple(w.shape)}, expected (7, 7)")
    return w.detach().to(device=dev, dtype=torch.float64).reshape(49).contiguous()


def _niqe_features(x, shave, win, sizes, keep=None):
    """fp64 [N, nb, 36] on the device: dsr_niqe_plane, dsr_imresize_f32 (x0.5), dsr_niqe_moments per scale, dsr_niqe_features.
    `keep` (a dict) receives the intermediate tensors."""
    n, h, w, hc, wc = sizes
    dt, xx = _luma_in(x)
    plane = torch.empty(n, hc, wc, dtype=torch.float32, device=x.device)
    check(_lib.lib().dsr_niqe_plane(dt, _ptr(xx), n, 3, h, w, shave, _ptr(plane), _stream()))
    return _niqe_from_plane(plane, win, keep)


def _niqe_from_plane(plane, win, keep=None):
    """The passes behind dsr_niqe_plane on a contiguous fp32 [N, hc, wc] plane whose sides are multiples of 96."""
    from .functional import _imresize_launch
    from .utils.imresize import imresize_tables
    n, hc, wc = plane.shape
    lib = _lib.lib()
    dev = plane.device
    st = _stream()
    th = imresize_tables(hc, hc // 2, 0.5, "bicubic", True, dev)
    tw = imresize_tables(wc, wc // 2, 0.5, "bicubic", True, dev)
    half = torch.empty(n, hc // 2, wc // 2, dtype=torch.float32, device=dev)
    _imresize_launch(plane, half, n, hc, wc, hc // 2, wc // 2, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)
    nb = (hc // _NIQE_BLOCK) * (wc // _NIQE_BLOCK)
    m1 = torch.empty(n, nb, 5, 5, dtype=torch.float64, device=dev)
    m2 = torch.empty(n, nb, 5, 5, dtype=torch.float64, device=dev)
    check(lib.dsr_niqe_moments(_ptr(plane), n, hc, wc, _NIQE_BLOCK, _ptr(win), _ptr(m1), st))
    check(lib.dsr_niqe_moments(_ptr(half), n, hc // 2, wc // 2, _NIQE_BLOCK // 2, _ptr(win), _ptr(m2), st))
    feat = torch.empty(n, nb, _NIQE_FEATS, dtype=torch.float64, device=dev)
    check(lib.dsr_niqe_features(_ptr(m1), _ptr(m2), n, nb, _ptr(_niqe_device_tables(dev)), _ptr(feat), st))
    if keep is not None:
        keep.update(plane=plane, half=half, m1=m1, m2=m2)
    return feat


def niqe_features(x, shave=0, window=None):
    """fp64 [N, blocks, 36] on the device: the NIQE feature table of an [N, 3, H, W] tensor in [0, 1] (fp32, fp16 or bf16, read
    as it is) -- see ``NaturalnessImageQualityEvaluator`` for the definition.  ``window``: a [7, 7] array or tensor, default the
    published Gaussian (sigma 7/6).  Blocks are in row-major order; scale 1's 18 features come first.  Nothing is read on the
    host.  PARITY UNPINNED."""
    shave = _check_shave("niqe_features", shave)
    if window is not None:
        window = window if torch.is_tensor(window) else torch.as_tensor(window)
        if tuple(window.shape) != (7, 7):
            raise ValueError(f"niqe_features: the window has shape {tuple(window.shape)}, expected (7, 7)")
    sizes = _niqe_check("niqe_features", x, shave)
    return _niqe_features(x, shave, _niqe_window(window, x.device), sizes)


def niqe_statistics(feat):
    """fp64 [N, 36 + 36 * 36 + 1] on the device from a feature table [N, nb, 36]: per image the column-wise ``nanmean``, the
    ``np.cov(rowvar=False)`` (ddof 1) of the rows without a NaN, and the number of those rows.  Torch device ops in float64
    (elementwise and ``sum`` only, nothing read on the host).  Fewer than two such rows leave a non-finite covariance."""
    n, nb, f = feat.shape
    mu = torch.nanmean(feat, dim=1)
    good = ~torch.isnan(feat).any(dim=2)                                   # [N, nb]
    cnt = good.sum(dim=1).to(torch.float64)                                # [N]
    z = torch.where(good[:, :, None], feat, torch.zeros((), dtype=feat.dtype, device=feat.device))
    mean = z.sum(dim=1) / cnt[:, None]
    d = torch.where(good[:, :, None], z - mean[:, None, :], torch.zeros((), dtype=feat.dtype, device=feat.device))
    cov = (d[:, :, :, None] * d[:, :, None, :]).sum(dim=1) / (cnt - 1.0)[:, None, None]
    return torch.cat([mu, cov.reshape(n, f * f), cnt[:, None]], dim=1)


def niqe_score(stats, mu_p, cov_p):
    """float64 numpy [N] from the HOST copy of ``niqe_statistics``: sqrt((mu_p - mu_d) pinv((cov_p + cov_d) / 2) (mu_p -
    mu_d)^T) per image; NaN (no exception) where fewer than two blocks are NaN-free or a feature column is NaN throughout."""
    import numpy as np
    stats = np.asarray(stats, dtype=np.float64)
    out = np.full(stats.shape[0], np.nan)
    for i, row in enumerate(stats):
        mu_d, cov_d, cnt = row[:36], row[36:36 + 1296].reshape(36, 36), row[-1]
        if cnt < 2 or not np.isfinite(mu_d).all() or not np.isfinite(cov_d).all():
            continue
        d = mu_p.reshape(1, 36) - mu_d.reshape(1, 36)
        out[i] = float(np.sqrt(d @ np.linalg.pinv((cov_p + cov_d) / 2.0) @ d.T).item())
    return out


class NaturalnessImageQualityEvaluator(nn.Module):
    """NIQE (Mittal, Soundararajan, Bovik 2013), the no-reference score real-world super-resolution is reported by (Real-ESRGAN;
    BasicSR ``calculate_niqe``), on the HIP path -- PARITY UNPINNED: BasicSR, OpenCV and ``niqe_pris_params.npz`` are not
    installed here, the formulas are BasicSR's, restated; the float64 statement is tests/niqe_ref.py.  Lower is better.

    Per image of ``preds`` ([N, 3, H, W] in [0, 1]; fp32, fp16 or bf16, read as it is):
      1. each channel becomes its 8-bit code, ``shave`` pixels are cut from each border, ``Y = round_half_even(16 + (65481 r +
         128553 g + 24966 b) / 255000)`` in integer arithmetic, and the plane is cropped at the bottom and right to multiples of
         96; at least two 96 x 96 blocks must remain (ValueError otherwise);
      2. at scale 1 on that plane and at scale 2 on its MATLAB-style bicubic antialiased x0.5 (``dsr_imresize_f32``), with the
         7 x 7 window w over replicated borders: ``mu = w (*) x``, ``sigma = sqrt(|w (*) x^2 - mu^2|)``, ``v = (x - mu) /
         (sigma + 1)``, in float64.  The resize runs on the plane in its 0..255 scale and in fp32, which is exact there (the
         x0.5 weights are (-3, -9, 29, 111, 111, 29, -9, -3) / 256: 8 + 8 + 8 bits); BasicSR resizes ``img / 255`` in float64
         and multiplies back: the operator is linear, so the two differ by rounding only -- which can still move an alpha by
         one grid step;
      3. per 96 x 96 block (48 x 48 at scale 2) an asymmetric generalised Gaussian is fitted to v and to its products with the
         neighbour rolled by (0, 1), (1, 0), (1, 1), (1, -1) inside the block: 18 features per scale, 36 per block.  A map with
         no negative or no positive element (a flat block) takes alpha = 0.2 with NaN betas, as ``np.argmin`` of NaNs does;
      4. ``mu_d`` = the column-wise nanmean of the [blocks, 36] table, ``cov_d`` = the covariance (ddof 1) of its NaN-free rows,
         ``NIQE = sqrt((mu_p - mu_d) pinv((cov_p + cov_d) / 2) (mu_p - mu_d)^T)``; NaN when fewer than two rows are NaN-free.
    Inside a textured block a flat neighbourhood leaves x - mu as rounding residue, whose sign then counts in the fit; BasicSR has
    the same property and nothing here hides it.

    ``params``: a path to a local ``.npz`` with ``mu_pris_param`` [1, 36], ``cov_pris_param`` [36, 36] and ``gaussian_window``
    [7, 7] (BasicSR's file as it is), or a ``(mu, cov, window)`` tuple.  ``None`` uses stand-ins -- ``mu_p = 0``, ``cov_p = I`` and
    the published sigma = 7/6 window -- and warns once: such scores rank images under the same stand-ins but are NOT comparable
    with published NIQE numbers.  ``reduction``: 'elementwise_mean', 'sum' or 'none' / None.

    ``update`` launches the device work (five launches and a few float64 torch ops for the statistics) and reads nothing on the
    host; ``compute`` / ``forward`` copy ``36 + 36^2 + 1`` numbers per image to the host once and take the pseudo-inverse there
    in numpy, so their result is a HOST float64 tensor.  Not differentiable."""

    def __init__(self, params=None, shave=0, reduction="elementwise_mean"):
        super().__init__()
        global _niqe_warned
        name = type(self).__name__
        self.shave = _check_shave(name, shave)
        self.reduction = _check_reduction(name, reduction)
        self.pretrained = params is not None
        if params is None:
            import numpy as np
            self.mu_p, self.cov_p, self.window = np.zeros((1, 36)), np.eye(36), None
            if not _niqe_warned:
                _niqe_warned = True
                import warnings
                warnings.warn("NaturalnessImageQualityEvaluator: no `params` given; using stand-ins (mu = 0, cov = I, the "
                              "sigma = 7/6 window). Scores are not comparable with published NIQE numbers; pass BasicSR's "
                              "niqe_pris_params.npz.", stacklevel=2)
        else:
            self.mu_p, self.cov_p, self.window = load_niqe_params(params)
        self._stats = []

    def reset(self):
        self._stats = []

    def statistics(self, preds):
        """fp64 [N, 36 + 36^2 + 1] on the device (``niqe_statistics`` of the batch's features); the running state is not
        touched and nothing is read on the host.  ``niqe_score(stats.cpu().numpy(), self.mu_p, self.cov_p)`` turns any stack
        of these into scores: how ``evaluate_generator`` crosses to the host once after its loop."""
        sizes = _niqe_check(type(self).__name__, preds, self.shave)
        return niqe_statistics(_niqe_features(preds, self.shave, _niqe_window(self.window, preds.device), sizes))

    def _batch(self, preds):
        stats = self.statistics(preds)
        self._stats.append(stats)
        return stats

    def _reduce(self, stats):
        scores = torch.from_numpy(niqe_score(stats.cpu().numpy(), self.mu_p, self.cov_p))
        if self.reduction == "none":
            return scores
        return scores.sum() if self.reduction == "sum" else scores.mean()

    def update(self, preds):
        self._batch(preds)

    def forward(self, preds):
        return self._reduce(self._batch(preds))

    def compute(self):
        if not self._stats:
            raise RuntimeError(f"{type(self).__name__}.compute() called before update()")
        return self._reduce(torch.cat(self._stats))


NIQE = NaturalnessImageQualityEvaluator
