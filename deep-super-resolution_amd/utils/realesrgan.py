"""The second-order degradation of Real-ESRGAN (BasicSR ``RealESRGANModel.feed_data``) on the device, and its training-pair pool.

``RealESRGANDegradation`` turns a ground-truth batch into its low-quality input: blur from the mixed kernel family, a random
resize, Gaussian or Poisson noise and a JPEG round trip, the same chain a second time, then a final resize with a sinc filter in
either order with the last JPEG.  It is the stage functions of ``utils.degradation`` (``filter2d``, ``add_gaussian_noise_batch``,
``add_poisson_noise_batch``, ``jpeg_batch``) and ``utils.imresize.interpolate`` called one after another with the values of a
``DegradationPlan``; the pipeline adds no arithmetic of its own but the last rounding to grey levels.  Every random choice
but the noise draws is made on the host by ``plan`` from a numpy generator, so a seeded plan repeats; the noise draws come
from torch on the device.  Parity with BasicSR is unpinned (BasicSR, OpenCV and torchvision were not available): the
definitions are the ones written out in the docstrings here, and JPEG qualities are whole numbers (``jpeg_batch`` is Pillow's
codec, not DiffJPEG).
"""
import math

import numpy as np
import torch

from . import degradation as D
from .imresize import interpolate, interpolate_out_size

KERNEL_PAD = 21
KERNEL_SIZES = tuple(range(7, 22, 2))
RESIZE_MODES = ("area", "bilinear", "bicubic")
KERNEL_PROB = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)


class DegradationPlan:
    """Every draw of one degraded batch, a plain object.  Kernels: ``kernel1``, ``kernel2``, ``sinc_kernel``, fp32 numpy
    [B, 21, 21] (``sinc_kernel`` is a delta for a sample whose final sinc filter is not drawn).  Per batch: ``scale1``,
    ``mode1``, ``scale2``, ``mode2``, ``mode3`` (resize factors and modes), ``second_blur``, ``noise1`` / ``noise2``
    ("gaussian" or "poisson"), ``jpeg_last`` (True: resize, sinc filter, then JPEG; False: JPEG first).  Per sample, numpy
    [B]: ``amount1`` / ``amount2`` (the Gaussian sigma in 0..255 units or the Poisson scale), ``gray1`` / ``gray2`` (bool),
    ``quality1`` (the first JPEG) / ``quality2`` (the last) (int).  Sizes (h, w): ``size1`` after the first resize, ``size2`` after the second,
    ``size3`` the output."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        keep = {k: v for k, v in self.__dict__.items() if not k.startswith("kernel") and k != "sinc_kernel"}
        return f"DegradationPlan({keep})"


class RealESRGANDegradation:
    """The published x4plus option values by default.  First stage: `resize_prob` (up, down, keep) and `resize_range`,
    `gaussian_noise_prob` (otherwise Poisson), `noise_range` (sigma, 0..255 units), `poisson_scale_range`, `gray_noise_prob`,
    `jpeg_range` (whole qualities, both ends included).  Second stage: `second_blur_prob` and the same names with a 2.  Kernels:
    `kernel_list` / `kernel_prob` / `kernel_sizes` / `blur_sigma` / `betag_range` / `betap_range` / `sinc_prob` (and the 2s) as
    ``degradation.random_mixed_kernels``; `final_sinc_prob`; `jpeg_subsampling` as ``jpeg_batch``."""

    def __init__(self, scale=4, resize_prob=(0.2, 0.7, 0.1), resize_range=(0.15, 1.5), gaussian_noise_prob=0.5, noise_range=(1, 30),
                 poisson_scale_range=(0.05, 3), gray_noise_prob=0.4, jpeg_range=(30, 95), second_blur_prob=0.8,
                 resize_prob2=(0.3, 0.4, 0.3), resize_range2=(0.3, 1.2), gaussian_noise_prob2=0.5, noise_range2=(1, 25),
                 poisson_scale_range2=(0.05, 2.5), gray_noise_prob2=0.4, jpeg_range2=(30, 95), kernel_list=D.KERNEL_LIST,
                 kernel_prob=KERNEL_PROB, kernel_sizes=KERNEL_SIZES, blur_sigma=(0.2, 3), betag_range=(0.5, 4), betap_range=(1, 2),
                 sinc_prob=0.1, kernel_list2=D.KERNEL_LIST, kernel_prob2=KERNEL_PROB, blur_sigma2=(0.2, 1.5), betag_range2=(0.5, 4),
                 betap_range2=(1, 2), sinc_prob2=0.1, final_sinc_prob=0.8, jpeg_subsampling="4:2:0"):
        self.scale = int(scale)
        if self.scale < 1:
            raise ValueError(f"RealESRGANDegradation: scale {scale}")
        for name, p in (("resize_prob", resize_prob), ("resize_prob2", resize_prob2)):
            if len(p) != 3 or min(p) < 0 or not sum(p) > 0:
                raise ValueError(f"RealESRGANDegradation: {name} {p} is not three non-negative weights (up, down, keep)")
        for name, r in (("resize_range", resize_range), ("resize_range2", resize_range2)):
            if not 0 < r[0] <= 1 <= r[1]:
                raise ValueError(f"RealESRGANDegradation: {name} {r} is not 0 < low <= 1 <= high")
        for name, q in (("jpeg_range", jpeg_range), ("jpeg_range2", jpeg_range2)):
            if len(q) != 2 or not all(D._is_int(v) for v in q) or not 1 <= q[0] <= q[1] <= 100:
                raise ValueError(f"RealESRGANDegradation: {name} {q} is not (low, high) with integers 1 <= low <= high <= 100")
        D._subsampling(jpeg_subsampling)
        self.stage = (
            dict(resize_prob=tuple(resize_prob), resize_range=tuple(resize_range), gaussian_noise_prob=float(gaussian_noise_prob),
                 noise_range=tuple(noise_range), poisson_scale_range=tuple(poisson_scale_range), gray_noise_prob=float(gray_noise_prob),
                 jpeg_range=tuple(jpeg_range)),
            dict(resize_prob=tuple(resize_prob2), resize_range=tuple(resize_range2), gaussian_noise_prob=float(gaussian_noise_prob2),
                 noise_range=tuple(noise_range2), poisson_scale_range=tuple(poisson_scale_range2),
                 gray_noise_prob=float(gray_noise_prob2), jpeg_range=tuple(jpeg_range2)))
        self.kernels = (
            dict(kernel_list=tuple(kernel_list), kernel_prob=tuple(kernel_prob), sigma=tuple(blur_sigma), betag=tuple(betag_range),
                 betap=tuple(betap_range), sinc_prob=float(sinc_prob)),
            dict(kernel_list=tuple(kernel_list2), kernel_prob=tuple(kernel_prob2), sigma=tuple(blur_sigma2), betag=tuple(betag_range2),
                 betap=tuple(betap_range2), sinc_prob=float(sinc_prob2)))
        self.kernel_sizes = tuple(int(s) for s in kernel_sizes)
        self.second_blur_prob, self.final_sinc_prob = float(second_blur_prob), float(final_sinc_prob)
        self.jpeg_subsampling = jpeg_subsampling

    # ------------------------------------------------------------------ the draws
    def _kernels(self, n, k, rng):
        return D.random_mixed_kernels(n, k["kernel_list"], k["kernel_prob"], self.kernel_sizes, k["sigma"], k["sigma"],
                                      (-math.pi, math.pi), k["betag"], k["betap"], k["sinc_prob"], rng, KERNEL_PAD)

    @staticmethod
    def _stage(n, st, low, rng):
        """resize factor and mode, noise kind, then per sample amount, grey flag and JPEG quality"""
        up, down, _ = st["resize_prob"]
        u = float(rng.uniform(0.0, 1.0)) * sum(st["resize_prob"])
        lo, hi = st["resize_range"]
        lo = min(max(lo, low), 1.0)
        scale = float(rng.uniform(1.0, hi)) if u < up else (float(rng.uniform(lo, 1.0)) if u < up + down else 1.0)
        mode = RESIZE_MODES[int(rng.randint(len(RESIZE_MODES)))]
        kind = "gaussian" if float(rng.uniform(0.0, 1.0)) < st["gaussian_noise_prob"] else "poisson"
        a = st["noise_range"] if kind == "gaussian" else st["poisson_scale_range"]
        amount = rng.uniform(a[0], a[1], size=n).astype(np.float32)
        gray = rng.uniform(0.0, 1.0, size=n) < st["gray_noise_prob"]
        quality = rng.randint(st["jpeg_range"][0], st["jpeg_range"][1] + 1, size=n).astype(np.int32)
        return scale, mode, kind, amount, gray, quality

    def plan(self, batch, h, w, rng=None):
        """The ``DegradationPlan`` of a [batch, 3, h, w] ground-truth batch; h and w multiples of `scale` with at least 11
        output pixels each (what the 21 x 21 filters need to reflect).  All draws come from `rng` (numpy's global generator by
        default), in this order:
          1. ``kernel1`` and then ``kernel2``: ``random_mixed_kernels(batch, ...)`` with the first- and second-stage settings;
          2. ``sinc_kernel``, per sample: ``uniform(0, 1)`` < final_sinc_prob; if so ``randint`` picks the size among
             `kernel_sizes` and ``uniform(pi / 3, pi)`` the cutoff (``sinc_kernel`` padded to 21), otherwise a delta;
          3. first stage: ``uniform(0, 1)`` picks up / down / keep by `resize_prob` and, unless keep, ``uniform`` draws the
             factor in [1, high) or [low, 1); ``randint(3)`` the mode among area, bilinear, bicubic; ``uniform(0, 1)`` <
             gaussian_noise_prob the noise kind; then three vectors of `batch` draws: the amounts (uniform in `noise_range` or
             `poisson_scale_range`), the grey flags (uniform < gray_noise_prob), the qualities (randint over `jpeg_range`);
          4. ``uniform(0, 1)`` < second_blur_prob;
          5. second stage, as 3 with its own settings;
          6. ``randint(3)``: the mode of the final resize; ``uniform(0, 1)`` < 0.5: ``jpeg_last``.
        The second stage's qualities are those of the last JPEG (the chain has two JPEG passes).
        The low end of a shrinking factor is raised where a blurred intermediate would otherwise be shorter than 11 pixels
        (ground truth below 74 pixels at the default 0.15)."""
        rng = np.random if rng is None else rng
        batch, h, w = int(batch), int(h), int(w)
        need = KERNEL_PAD // 2 + 1
        if batch < 1 or h % self.scale or w % self.scale or min(h, w) // self.scale < need:
            raise ValueError(f"RealESRGANDegradation: a {batch}x3x{h}x{w} batch at scale {self.scale}: sizes must be multiples of the "
                             f"scale with at least {need} output pixels")
        kernel1 = self._kernels(batch, self.kernels[0], rng)
        kernel2 = self._kernels(batch, self.kernels[1], rng)
        sinc = np.zeros((batch, KERNEL_PAD, KERNEL_PAD), dtype=np.float32)
        for b in range(batch):
            if float(rng.uniform(0.0, 1.0)) < self.final_sinc_prob:
                ks = self.kernel_sizes[int(rng.randint(len(self.kernel_sizes)))]
                sinc[b] = D.sinc_kernel(float(rng.uniform(math.pi / 3, math.pi)), ks, KERNEL_PAD)
            else:
                sinc[b, KERNEL_PAD // 2, KERNEL_PAD // 2] = 1.0
        scale1, mode1, noise1, amount1, gray1, quality1 = self._stage(batch, self.stage[0], (need + 0.5) / min(h, w), rng)
        second_blur = float(rng.uniform(0.0, 1.0)) < self.second_blur_prob
        scale2, mode2, noise2, amount2, gray2, quality2 = self._stage(batch, self.stage[1], 0.0, rng)
        mode3 = RESIZE_MODES[int(rng.randint(len(RESIZE_MODES)))]
        jpeg_last = float(rng.uniform(0.0, 1.0)) < 0.5
        size1 = (interpolate_out_size(h, scale_factor=scale1), interpolate_out_size(w, scale_factor=scale1))
        size2 = (max(1, int(h / self.scale * scale2)), max(1, int(w / self.scale * scale2)))
        size3 = (h // self.scale, w // self.scale)
        return DegradationPlan(kernel1=kernel1, kernel2=kernel2, sinc_kernel=sinc, scale1=scale1, mode1=mode1, scale2=scale2,
                               mode2=mode2, mode3=mode3, second_blur=second_blur, noise1=noise1, noise2=noise2, jpeg_last=jpeg_last,
                               amount1=amount1, gray1=gray1, quality1=quality1, amount2=amount2, gray2=gray2, quality2=quality2,
                               size1=size1, size2=size2, size3=size3)

    # ------------------------------------------------------------------ the stages in sequence
    @staticmethod
    def _noise(x, kind, amount, gray, generator):
        amount = torch.from_numpy(np.ascontiguousarray(amount, dtype=np.float32))
        gray = torch.from_numpy(np.ascontiguousarray(gray, dtype=np.uint8))
        fn = D.add_gaussian_noise_batch if kind == "gaussian" else D.add_poisson_noise_batch
        return fn(x, amount, gray, generator=generator)

    def __call__(self, gt, plan=None, generator=None, rng=None):
        """gt: fp32 [B, 3, H, W] device batch in [0, 1] -> lq: fp32 [B, 3, H / scale, W / scale] on the k / 255 grid.  `plan`: a
        ``DegradationPlan`` (default: ``self.plan(B, H, W, rng)``); `generator`: the torch.Generator of the noise draws.  In order:
        filter2d(kernel1), interpolate(scale_factor=scale1, mode1), first-stage noise, jpeg_batch(quality1), optionally
        filter2d(kernel2), interpolate(size=size2, mode2), second-stage noise, then either interpolate(size=size3, mode3),
        filter2d(sinc_kernel), jpeg_batch(quality2) or the JPEG first, and at the end round(clamp(x, 0, 1) * 255) / 255."""
        if not (torch.is_tensor(gt) and gt.dtype == torch.float32 and gt.dim() == 4 and gt.shape[1] == 3):
            raise TypeError("RealESRGANDegradation: an fp32 [B, 3, H, W] tensor is expected")
        D._need_gpu(gt)
        b, _, h, w = (int(v) for v in gt.shape)
        p = self.plan(b, h, w, rng) if plan is None else plan
        ss = self.jpeg_subsampling
        out = D.filter2d(gt, p.kernel1)
        out = interpolate(out, scale_factor=p.scale1, mode=p.mode1)
        out = self._noise(out, p.noise1, p.amount1, p.gray1, generator)
        out = D.jpeg_batch(out, p.quality1, ss)
        if p.second_blur:
            out = D.filter2d(out, p.kernel2)
        out = interpolate(out, size=p.size2, mode=p.mode2)
        out = self._noise(out, p.noise2, p.amount2, p.gray2, generator)
        if p.jpeg_last:
            out = interpolate(out, size=p.size3, mode=p.mode3)
            out = D.filter2d(out, p.sinc_kernel)
            out = D.jpeg_batch(out, p.quality2, ss)
        else:
            out = D.jpeg_batch(out, p.quality2, ss)
            out = interpolate(out, size=p.size3, mode=p.mode3)
            out = D.filter2d(out, p.sinc_kernel)
        return torch.round(torch.clamp(out, 0.0, 1.0) * 255.0) / 255.0


class PairPool:
    """BasicSR's ``_dequeue_and_enqueue``: a pool of `size` (lq, gt) pairs that decorrelates the degradations within a batch
    (a batch shares its resize factors and noise kinds).  Until the pool is full a batch is stored and returned as it came.
    From then on every call shuffles the pool with a seeded permutation, hands out its first B entries and puts the incoming
    batch in their place.  The pool lives on the device of the first batch; the permutation is made on the host and uploaded,
    nothing is read back.  `size` must be a multiple of the batch size."""

    def __init__(self, size=180, seed=0):
        self.size = int(size)
        if self.size < 1:
            raise ValueError(f"PairPool: size {size}")
        self.generator = torch.Generator().manual_seed(int(seed))
        self.lq = self.gt = None
        self.filled = 0

    def __call__(self, lq, gt):
        b = int(lq.shape[0])
        if gt.shape[0] != b or b < 1 or self.size % b:
            raise ValueError(f"PairPool: a batch of {b} and {gt.shape[0]} for a pool of {self.size}")
        if self.lq is None:
            self.lq = torch.zeros((self.size,) + tuple(lq.shape[1:]), dtype=lq.dtype, device=lq.device)
            self.gt = torch.zeros((self.size,) + tuple(gt.shape[1:]), dtype=gt.dtype, device=gt.device)
        if tuple(lq.shape[1:]) != tuple(self.lq.shape[1:]) or tuple(gt.shape[1:]) != tuple(self.gt.shape[1:]):
            raise ValueError("PairPool: the shape of a pair changed")
        if self.filled < self.size:
            self.lq[self.filled:self.filled + b] = lq
            self.gt[self.filled:self.filled + b] = gt
            self.filled += b
            return lq, gt
        perm = torch.randperm(self.size, generator=self.generator).to(self.lq.device)
        self.lq, self.gt = self.lq[perm], self.gt[perm]
        out = self.lq[:b].clone(), self.gt[:b].clone()
        self.lq[:b] = lq
        self.gt[:b] = gt
        return out
