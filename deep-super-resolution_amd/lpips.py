"""LPIPS with the AlexNet trunk on the HIP path: the metric the reference's scripts log next to PSNR and SSIM
(torchmetrics ``LearnedPerceptualImagePatchSimilarity(net_type='alex')``: train_GAN.py:8,32,112,131, eval_GAN.py:7,32,49,66,
DIP.py:8,75,120,159,185).

torchmetrics and the lpips package are absent here, so the definition is restated from its publication (Zhang et al. 2018,
"The Unreasonable Effectiveness of Deep Features as a Perceptual Metric") and torchmetrics' documented behaviour -- PARITY
UNPINNED, as for PSNR (evaluate.py):
  1. img1, img2: fp32 [N,3,H,W] in [-1,1] (or [0,1] with ``normalize=True``, mapped by x -> 2x - 1);
  2. scaling layer (x - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450);
  3. torchvision ``alexnet().features``: Conv(3,64,11,s4,p2) ReLU | MaxPool(3,2) Conv(64,192,5,p2) ReLU | MaxPool(3,2)
     Conv(192,384,3,p1) ReLU | Conv(384,256,3,p1) ReLU | Conv(256,256,3,p1) ReLU, tapped after each ReLU;
  4. per tap k: channel-normalise each pixel with torchmetrics' form f / sqrt(1e-8 + sum_c f^2) (the lpips package divides by
     sqrt(sum f^2) + 1e-10 instead; the two differ only for near-zero feature vectors), then
     d_k = mean_{h,w} sum_c w_k[c] (n1_c - n2_c)^2 with the 1x1 ``lin{k}`` weight (no bias; its dropout is a no-op in eval);
  5. per image sum_k d_k; the batch mean (``reduction='mean'``) or sum.

Device work (csrc/lpips.hip, include/dsr_hip.h): one stem-preparation launch for both images (scaling, padding, 4x4
space-to-depth to 64 channels, input range), the five convolutions on dsr_conv_fwd with a bias + ReLU epilogue (16-bit storage,
fp32 accumulation; the batch of 2N images runs the trunk once), two 3x3 / stride-2 max-pool launches, one distance launch for
all five taps and one finalise launch.  Only the [N] / scalar result and the input's (min, max) key pair leave the device.

Backward (LPIPS as a training loss, ``loss = l1 + 0.1 * lpips(fake, hr)``): when grad mode is on and an input requires a
gradient, the call goes through one autograd node that keeps the five tap tensors and runs, per trunk pass,
  dsr_lpips_distance_bwd   the distance's closed-form derivative at all five taps, times each tap's ReLU mask;
  dsr_conv_dgrad_masked    conv5 and conv4 (the mask of relu4 / relu3 in the epilogue) + dsr_pw_add of that tap's distance part;
  dsr_conv_dgrad           conv3, conv2 and the stem (as the 3x3 / pad-0 conv over the space-to-depth input);
  dsr_maxpool3s2_bwd       twice: pool backward + ReLU mask + the distance part of relu2 / relu1 in one pass;
  dsr_lpips_stem_prep_bwd  16-bit gradient of the stem input -> fp32 NCHW image gradient.
The weights are frozen buffers: there is no weight gradient.  If only one image requires a gradient (the training case: img2 is
the HR target) every launch after the first covers that half of the batch only.  Nothing on the path reads a device value on
the host; with ``validate_range=False`` the forward does not either, and forward + backward can be captured in a HIP graph.

The 11x11 / stride-4 stem has 121 taps, more than the conv kernels take; after the space-to-depth it is an exact 3x3 / stride-1
/ pad-0 conv over 64 channels (48 real + 16 zero), whose weight is the 11x11 kernel zero-padded to 12x12 and regrouped once on
the host (``stem_weight_s2d``).  64 rather than 48 input channels keep the conv on the gather kernels' 64-channel fast path.

Weights: the trained numbers need torchvision's AlexNet checkpoint and the lpips package's ``alex.pth`` heads, which cannot be
downloaded here.  Like ``Vgg19Loss(state_dict=...)``, ``LPIPS(net_weights=..., lin_weights=...)`` takes them from local files
(or state dicts) the caller provides; otherwise deterministic stand-ins are used and ``pretrained`` is False.
"""
import ctypes as C
import math
import os
import struct
from collections.abc import Mapping

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import ACT_RELU, BF16, F16, PAD_ZERO, ConvDesc, Epilogue, _ptr, _stream, check

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# torchvision alexnet().features: (index, Cout, Cin, kernel, stride, padding) of the five convolutions
ALEX_CONVS = ((0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1))
LIN_CHANNELS = (64, 192, 384, 256, 256)
STEM_CP = 64                       # channels of the space-to-depth stem input (48 real)
_MAX_BYTES = (1 << 31) - 1         # dsr_conv_fwd takes tensors below 2 GiB


def stem_weight_s2d(w):
    """[O,3,11,11] stem weight -> [O,64,3,3]: zero-padded to 12x12, tap (4by+py, 4bx+px) of channel c moved to channel
    (py*4 + px)*3 + c of tap (by, bx); channels 48..63 are zero.  A 3x3 valid conv of this weight over the 4x4 space-to-depth
    of the padded input equals the 11x11 / stride-4 conv."""
    o = w.shape[0]
    w12 = torch.zeros(o, 3, 12, 12, dtype=w.dtype)
    w12[:, :, :11, :11] = w
    t = w12.view(o, 3, 3, 4, 3, 4).permute(0, 3, 5, 1, 2, 4).reshape(o, 48, 3, 3)     # [o][py][px][c][by][bx]
    out = torch.zeros(o, STEM_CP, 3, 3, dtype=w.dtype)
    out[:, :48] = t
    return out


# ----------------------------------------------------------------------------- weights
def _standin_alex_state(seed=4321):
    """Deterministic AlexNet ``features`` weights: He-uniform so that activations keep O(1) scale (as _standin_vgg_state)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cout, cin, k, _, _ in ALEX_CONVS:
        bound = float(np.sqrt(6.0 / (cin * k * k)))
        sd[f"{idx}.weight"] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        sd[f"{idx}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.05
    return sd


def _standin_lin_state(seed=4322):
    """Deterministic non-negative 1x1 heads (trained LPIPS heads are non-negative)."""
    g = torch.Generator().manual_seed(seed)
    return {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) * (8.0 / c) for k, c in enumerate(LIN_CHANNELS)}


def _as_state(obj, what):
    if isinstance(obj, (str, os.PathLike)):
        obj = torch.load(obj, map_location="cpu", weights_only=True)
    if not isinstance(obj, Mapping):
        raise TypeError(f"LPIPS: {what} must be a path or a state dict, got {type(obj).__name__}")
    return obj


_SLICE = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}      # lpips package: features[0:2] -> slice1, [2:5] -> slice2, ... [10:12] -> slice5
_NET_LAYOUTS = ("features.{i}.{p}", "{i}.{p}", "net.slice{s}.{i}.{p}")


def _get(sd, key, shape, what):
    if key not in sd:
        raise RuntimeError(f"LPIPS: {what} has no '{key}'")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError(f"LPIPS: {what} '{key}' has shape {got}, expected {tuple(shape)}")
    return t.detach().to("cpu", torch.float32)


def load_net_state(obj):
    """AlexNet ``features`` weights from a path or state dict in any of three layouts -- torchvision ``alexnet()``
    (``features.{0,3,6,8,10}.*``; ``classifier.*`` is ignored), its ``features`` sub-dict (``{0,3,6,8,10}.*``) or the lpips
    package's ``net.slice{1..5}.{i}.*`` -- as ``{'{i}.weight': .., '{i}.bias': ..}`` fp32.  A missing key or a wrong shape
    raises RuntimeError naming the key."""
    sd = _as_state(obj, "net_weights")
    want = [(i, s, p) for i, s in _SLICE.items() for p in ("weight", "bias")]
    # the layout under which most of the ten keys exist (a dict with none of them is named in the torchvision layout)
    layout = max(_NET_LAYOUTS, key=lambda f: sum(f.format(i=i, s=s, p=p) in sd for i, s, p in want))
    out = {}
    for idx, cout, cin, k, _, _ in ALEX_CONVS:
        s = _SLICE[idx]
        out[f"{idx}.weight"] = _get(sd, layout.format(i=idx, s=s, p="weight"), (cout, cin, k, k), "net_weights")
        out[f"{idx}.bias"] = _get(sd, layout.format(i=idx, s=s, p="bias"), (cout,), "net_weights")
    return out


def load_lin_state(obj):
    """The five 1x1 heads ``lin{0..4}.model.1.weight`` ([1,C,1,1], the lpips package's ``alex.pth``) as fp32 [C] tensors."""
    sd = _as_state(obj, "lin_weights")
    return [_get(sd, f"lin{k}.model.1.weight", (1, c, 1, 1), "lin_weights").reshape(c) for k, c in enumerate(LIN_CHANNELS)]


def _decode_key(k):
    """Inverse of order_key (csrc/dsr_common.h): order-preserving unsigned key -> float."""
    k &= 0xFFFFFFFF
    bits = (k ^ 0x80000000) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# ----------------------------------------------------------------------------- the module
class LPIPS(nn.Module):
    """``LearnedPerceptualImagePatchSimilarity(net_type='alex', reduction, normalize)`` on the HIP path.

    ``forward(img1, img2)`` -> 0-dim fp32 device tensor (``.item()`` works as in the reference); ``per_image`` -> [N];
    ``update`` / ``compute`` / ``reset`` keep a running sum and image count on the device (torchmetrics' ``sum_scores`` /
    ``total``).  ``net_weights`` / ``lin_weights``: path or state dict (see load_net_state / load_lin_state); stand-ins
    otherwise.  ``dtype``: 16-bit storage of the trunk (fp32 accumulation).  ``validate_range=False`` skips the range check and
    with it the call's one host read (needed inside a captured graph).  ``grad_scale``: static loss scale of the 16-bit
    gradients (a power of two; None: chosen from the shapes, see ``_grad_scale``).

    ``forward`` and ``per_image`` are differentiable with respect to either image; ``update`` never is (as in torchmetrics)."""

    def __init__(self, net_type="alex", reduction="mean", normalize=False, net_weights=None, lin_weights=None,
                 dtype=torch.float16, validate_range=True, grad_scale=None):
        super().__init__()
        if net_type in ("vgg", "squeeze"):
            raise NotImplementedError(f"LPIPS: net_type '{net_type}' is not built here; only 'alex' is")
        if net_type != "alex":
            raise ValueError(f"LPIPS: net_type must be one of 'alex', 'vgg', 'squeeze', got {net_type!r}")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"LPIPS: reduction must be 'mean' or 'sum', got {reduction!r}")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"LPIPS: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        if grad_scale is not None and not (float(grad_scale) > 0 and math.isfinite(float(grad_scale))):
            raise ValueError(f"LPIPS: grad_scale must be a positive finite number, got {grad_scale!r}")
        self.net_type, self.reduction, self.normalize, self.dtype = net_type, reduction, bool(normalize), dtype
        self.validate_range = bool(validate_range)
        self.grad_scale = None if grad_scale is None else float(grad_scale)
        self.pretrained = net_weights is not None and lin_weights is not None
        net = load_net_state(net_weights if net_weights is not None else _standin_alex_state())
        lin = load_lin_state(lin_weights if lin_weights is not None else _standin_lin_state())
        for k, (idx, *_rest) in enumerate(ALEX_CONVS):
            w = net[f"{idx}.weight"]
            self.register_buffer(f"w{k + 1}", stem_weight_s2d(w) if k == 0 else w.contiguous())
            self.register_buffer(f"b{k + 1}", net[f"{idx}.bias"].contiguous())
            self.register_buffer(f"lin{k + 1}", lin[k].contiguous())
        self.max_pairs_per_launch = None       # None: as many image pairs per trunk pass as keep every tensor below 2 GiB
        self._packed = {}
        self._packed_dgrad = {}
        self.reset()

    # ---- running state (torchmetrics Metric surface)
    def reset(self):
        self.sum_scores = None
        self.total = None
        self._count = 0

    def update(self, img1, img2):
        """Adds the batch's per-image values and its image count to the running state (after the inputs were validated)."""
        per, tot = self._run(img1, img2, 1.0)
        lib = _lib.lib()
        if self.sum_scores is None:
            self.sum_scores = torch.zeros(1, dtype=torch.float32, device=per.device)
            self.total = torch.zeros(1, dtype=torch.float32, device=per.device)
        one = torch.ones(1, dtype=torch.float32, device=per.device)
        check(lib.dsr_pw_axpby_f32(_ptr(self.sum_scores), _ptr(tot), 1.0, 1.0, None, _ptr(self.sum_scores), 1, _stream()))
        check(lib.dsr_pw_axpby_f32(_ptr(self.total), _ptr(one), 1.0, float(per.shape[0]), None, _ptr(self.total), 1, _stream()))
        self._count += per.shape[0]

    def compute(self):
        if self._count == 0:
            raise RuntimeError("LPIPS.compute() called before update()")
        out = torch.empty(1, dtype=torch.float32, device=self.sum_scores.device)
        scale = 1.0 / self._count if self.reduction == "mean" else 1.0      # (the count is mirrored on the host: no sync)
        check(_lib.lib().dsr_pw_axpby_f32(_ptr(self.sum_scores), None, scale, 0.0, None, _ptr(out), 1, _stream()))
        return out.reshape(())

    # ---- one-shot evaluation
    def forward(self, img1, img2):
        _, tot = self._run_or_apply(img1, img2)
        return tot.reshape(())

    def per_image(self, img1, img2):
        per, _ = self._run_or_apply(img1, img2)
        return per

    def _run_or_apply(self, img1, img2):
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (img1, img2)):
            self._check_inputs(img1, img2)
            return _LPIPSFunction.apply(self, img1, img2)
        return self._run(img1, img2, None)

    # ---- the device path
    def _check_inputs(self, img1, img2):
        for t in (img1, img2):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError("LPIPS: expected both inputs to be tensors of shape [N, 3, H, W], got "
                                 f"{tuple(img1.shape) if torch.is_tensor(img1) else type(img1).__name__} and "
                                 f"{tuple(img2.shape) if torch.is_tensor(img2) else type(img2).__name__}")
        if img1.shape != img2.shape:
            raise ValueError(f"LPIPS: the two inputs must have one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
        if not (img1.is_cuda and img2.is_cuda):
            raise RuntimeError("deep-super-resolution_amd: tensors must live on the MI355X (cuda device); "
                               "there is no CPU implementation of this path")

    def tap_sizes(self, h, w):
        """[(h, w)] of relu1..relu5 for an h x w image; RuntimeError naming the size if the trunk would produce an empty map."""
        out = (C.c_int * 10)()
        if _lib.lib().dsr_lpips_tap_sizes(int(h), int(w), out) != 0:
            raise RuntimeError(f"LPIPS: images of {h}x{w} are too small for the AlexNet trunk (an empty max-pool output; "
                               "height and width must be at least 31)")
        return [(out[2 * k], out[2 * k + 1]) for k in range(5)]

    def _weights(self, device):
        key = (str(device), self.dtype)
        hit = self._packed.get(key)
        if hit is not None:
            return hit
        if self.w1.device != device:
            self.to(device)
        lib = _lib.lib()
        dt = F16 if self.dtype == torch.float16 else BF16
        packed = []
        for k, (_, cout, cin, ks, _, _) in enumerate(ALEX_CONVS):
            w = getattr(self, f"w{k + 1}")
            cin_d, ks_d = (STEM_CP, 3) if k == 0 else (cin, ks)
            d = ConvDesc(dt, 1, 16, 16, cin_d, cout, ks_d, ks_d, 1, 0, PAD_ZERO)
            wf = torch.empty(lib.dsr_conv_packed_elems(C.byref(d), 0), dtype=self.dtype, device=device)
            check(lib.dsr_conv_pack_weight(C.byref(d), _ptr(w), _ptr(wf), None, _stream()))
            packed.append(wf)
        self._packed = {key: packed}
        return packed

    def _pairs_per_launch(self, h, w, sizes):
        bh, bw = sizes[0][0] + 2, sizes[0][1] + 2
        per_pair = max([2 * bh * bw * STEM_CP * 2] + [2 * y * x * c * 2 for (y, x), c in zip(sizes, LIN_CHANNELS)])
        pairs = _MAX_BYTES // per_pair
        if pairs < 1:
            raise RuntimeError(f"LPIPS: one {h}x{w} image pair needs a trunk tensor of 2 GiB or more")
        if self.max_pairs_per_launch is not None:
            pairs = min(pairs, int(self.max_pairs_per_launch))
        return max(pairs, 1)

    def _weights_dgrad(self, device):
        """The packed input-gradient weight images [tap][Cin][Cout], made at the first backward."""
        key = (str(device), self.dtype)
        hit = self._packed_dgrad.get(key)
        if hit is not None:
            return hit
        lib = _lib.lib()
        dt = F16 if self.dtype == torch.float16 else BF16
        packed = []
        for k, (_, cout, cin, ks, _, _) in enumerate(ALEX_CONVS):
            w = getattr(self, f"w{k + 1}")
            cin_d, ks_d = (STEM_CP, 3) if k == 0 else (cin, ks)
            d = ConvDesc(dt, 1, 16, 16, cin_d, cout, ks_d, ks_d, 1, 0, PAD_ZERO)
            wf = torch.empty(lib.dsr_conv_packed_elems(C.byref(d), 0), dtype=self.dtype, device=device)
            wd = torch.empty(lib.dsr_conv_packed_elems(C.byref(d), 1), dtype=self.dtype, device=device)
            check(lib.dsr_conv_pack_weight(C.byref(d), _ptr(w), _ptr(wf), _ptr(wd), _stream()))
            packed.append(wd)
        self._packed_dgrad = {key: packed}
        return packed

    def _total_scale(self, n):
        return 1.0 / n if self.reduction == "mean" else 1.0

    def _grad_scale(self, n, sizes):
        """The static loss scale S of the backward: every 16-bit gradient is S times the true one, the image gradient is
        divided by S again (dsr_lpips_stem_prep_bwd), so a power of two changes nothing but the range.

        Why it is needed: the distance gradient at tap k is 2 w (n1 - n2) / (s N hw_k) per element.  At the training size of the
        step recipes (32 pairs of 512 x 512: hw_1 = 127^2, hw_5 = 31^2) with w ~ 4 / C, |n1 - n2| ~ 0.1 / sqrt(C) and a feature
        norm s of a few units this is ~4e-9 at relu1 and ~1e-8 at relu5 -- below fp16's smallest subnormal (6e-8), four
        thousand times below its normal range (6.1e-5).  The elements scale with 1 / (N hw_1), so the default is
            S = 16 * 2^ceil(log2(N hw_1))        (N = 1 for reduction='sum': each image's value then has weight 1)
        which puts the typical relu1 element of an unrelated pair near 32 w |n1 - n2| / s ~ 1e-2 and the relu5 one (hw_1 / hw_5
        ~ 17 times larger) near 0.2, whatever the batch and image size: some 2^8 above fp16's normal limit and 2^16 below its
        maximum (a close pair, with |n1 - n2| ten times smaller, sits that much lower: see the measurement below).  The
        distance kernel saturates at the fp16 maximum instead of writing inf (a feature vector of norm ~1e-4 divides by it).
        bf16 storage has fp32's range; the same S is used and is harmless.  Measured on the MI355X at that size (stand-in
        weights, a noise-perturbed pair): unscaled, every element of all five taps rounds to zero in fp16; with the default
        S = 2^23 the medians are 3e-3 (relu1) and 2e-4 ... 6e-4 (relu2 ... relu5), the largest element 0.14, none is zero
        and 2 - 20 % per tap remain subnormal ("LPIPS backward")."""
        if self.grad_scale is not None:
            return self.grad_scale
        n_eff = n if self.reduction == "mean" else 1
        return float(2.0 ** (4 + math.ceil(math.log2(n_eff * sizes[0][0] * sizes[0][1]))))

    def _run(self, img1, img2, total_scale, keep=None):
        """(per_image [N], total [1]); total = total_scale * sum (None: the module's reduction).  Raises ValueError on
        out-of-range inputs before returning anything.  keep: a list that receives (first pair, last pair + 1, the five tap
        tensors) of every trunk pass, for the backward."""
        self._check_inputs(img1, img2)
        n, _, h, w = img1.shape
        sizes = self.tap_sizes(h, w)
        dev = img1.device
        img1 = img1.detach().contiguous().float()
        img2 = img2.detach().contiguous().float()
        wf = self._weights(dev)
        if total_scale is None:
            total_scale = self._total_scale(n)
        per = torch.empty(n, dtype=torch.float32, device=dev)
        tot = torch.empty(1, dtype=torch.float32, device=dev)
        rng = torch.zeros(2, dtype=torch.int32, device=dev)
        rng[:1].fill_(-1)                                         # min key 0xffffffff, max key 0 (a fill: no host copy)
        step = self._pairs_per_launch(h, w, sizes)
        for i0 in range(0, n, step):
            i1 = min(n, i0 + step)
            feats = self._trunk(img1[i0:i1], img2[i0:i1], sizes, wf, per[i0:i1], tot, total_scale, i0 > 0, rng)
            if keep is not None:
                keep.append((i0, i1, feats))
        if not self.validate_range:
            return per, tot
        lo_k, hi_k = rng.tolist()                                 # the one host read of the call
        lo, hi = _decode_key(lo_k), _decode_key(hi_k)
        lo_ok, hi_ok = (0.0, 1.0) if self.normalize else (-1.0, 1.0)
        if not (lo >= lo_ok and hi <= hi_ok):
            raise ValueError(f"LPIPS: expected both inputs to be normalized tensors with values in [{lo_ok:g}, {hi_ok:g}] "
                             f"(normalize={self.normalize}), got values in [{lo}, {hi}]")
        return per, tot

    def _trunk(self, img1, img2, sizes, wf, per, tot, total_scale, accumulate, rng):
        lib = _lib.lib()
        st = _stream()
        dt = F16 if self.dtype == torch.float16 else BF16
        n, _, h, w = img1.shape
        dev = img1.device
        bh, bw = sizes[0][0] + 2, sizes[0][1] + 2
        x = torch.empty((2 * n, bh, bw, STEM_CP), dtype=self.dtype, device=dev)
        check(lib.dsr_lpips_stem_prep(dt, _ptr(img1), _ptr(img2), n, h, w, int(self.normalize), _ptr(x), _ptr(rng), st))
        feats = []
        for k, (_, cout, cin, ks, _, pad) in enumerate(ALEX_CONVS):
            if k in (1, 2):                                       # MaxPool2d(3, 2) in front of conv2 and conv3
                _, ih, iw, cp = x.shape
                y = torch.empty((2 * n, (ih - 3) // 2 + 1, (iw - 3) // 2 + 1, cp), dtype=self.dtype, device=dev)
                check(lib.dsr_maxpool3s2_fwd(dt, _ptr(x), _ptr(y), 2 * n, ih, iw, cp, st))
                x = y
            cin_d, ks_d, pad_d = (STEM_CP, 3, 0) if k == 0 else (cin, ks, pad)
            _, ih, iw, _ = x.shape
            d = ConvDesc(dt, 2 * n, ih, iw, cin_d, cout, ks_d, ks_d, 1, pad_d, PAD_ZERO)
            oh, ow = sizes[k]
            y = torch.empty((2 * n, oh, ow, cout), dtype=self.dtype, device=dev)
            ep = Epilogue(ACT_RELU, 0.0, None, _ptr(getattr(self, f"b{k + 1}")), None, 0, None)
            check(lib.dsr_conv_fwd(C.byref(d), _ptr(x), _ptr(wf[k]), C.byref(ep), _ptr(y), st))
            feats.append(y)
            x = y
        hw = (C.c_int * 5)(*[y * x_ for y, x_ in sizes])
        cp = (C.c_int * 5)(*LIN_CHANNELS)
        blocks = lib.dsr_lpips_distance_blocks(5, hw, n)
        if blocks <= 0:
            raise RuntimeError(f"LPIPS: {n} image pairs of {h}x{w} are too many for one distance launch")
        partial = torch.empty(blocks, dtype=torch.float32, device=dev)
        fp = (C.c_void_p * 5)(*[f.data_ptr() for f in feats])
        lw = (C.c_void_p * 5)(*[getattr(self, f"lin{k + 1}").data_ptr() for k in range(5)])
        check(lib.dsr_lpips_distance(dt, 5, fp, lw, hw, cp, cp, n, _ptr(partial), st))
        check(lib.dsr_lpips_finalize(5, hw, n, _ptr(partial), _ptr(per), _ptr(tot), float(total_scale), int(accumulate), st))
        return feats

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

    def _dgrad(self, k, m, ih, iw, dy, wd, x_act=None):
        """Input gradient of conv k+1 over m images of ih x iw inputs; x_act: the ReLU output that is this conv's input, whose
        mask then rides in the launch's epilogue."""
        lib = _lib.lib()
        _, cout, cin, ks, _, pad = ALEX_CONVS[k]
        cin_d, ks_d, pad_d = (STEM_CP, 3, 0) if k == 0 else (cin, ks, pad)
        d = ConvDesc(F16 if self.dtype == torch.float16 else BF16, m, ih, iw, cin_d, cout, ks_d, ks_d, 1, pad_d, PAD_ZERO)
        dx = torch.empty((m, ih, iw, cin_d), dtype=self.dtype, device=dy.device)
        if x_act is None:
            check(lib.dsr_conv_dgrad(C.byref(d), _ptr(dy), _ptr(wd[k]), _ptr(dx), None, 0, _stream()))
        else:
            check(lib.dsr_conv_dgrad_masked(C.byref(d), _ptr(dy), _ptr(wd[k]), _ptr(x_act), ACT_RELU, 0.0, _ptr(dx), _stream()))
        return dx

    def _trunk_bwd(self, feats, n, h, w, sizes, g, which, out1, out2, scale):
        """Backward of one trunk pass.  feats: its five taps [2n]...; g: fp32 [n] upstream gradient per image; which: 1 = image
        1, 2 = image 2, 3 = both; out1 / out2: fp32 [n,3,h,w] slices that receive the image gradients."""
        lib = _lib.lib()
        st = _stream()
        dt = F16 if self.dtype == torch.float16 else BF16
        dev = feats[0].device
        wd = self._weights_dgrad(dev)
        m = 2 * n if which == 3 else n
        half = slice(n, 2 * n) if which == 2 else slice(0, m)       # the images the chain below runs on
        f = [t[half] for t in feats]
        dist = [torch.empty_like(t) for t in f]                     # the distance part of each tap's gradient
        hw = (C.c_int * 5)(*[y * x_ for y, x_ in sizes])
        cp = (C.c_int * 5)(*LIN_CHANNELS)
        fp = (C.c_void_p * 5)(*[t.data_ptr() for t in feats])
        lw = (C.c_void_p * 5)(*[getattr(self, f"lin{k + 1}").data_ptr() for k in range(5)])
        d1 = (C.c_void_p * 5)(*[t.data_ptr() for t in dist]) if which & 1 else None
        d2 = (C.c_void_p * 5)(*[t[m - n:].data_ptr() for t in dist]) if which & 2 else None
        check(lib.dsr_lpips_distance_bwd(dt, 5, fp, lw, hw, cp, cp, n, _ptr(g), float(scale), d1, d2, st))

        def add(a, b):
            out = torch.empty_like(a)
            check(lib.dsr_pw_add(dt, _ptr(a), _ptr(b), _ptr(out), a.numel() // 8, st))
            return out

        def pool_bwd(x, dy, addend):
            _, ih, iw, c = x.shape
            dx = torch.empty_like(x)
            check(lib.dsr_maxpool3s2_bwd(dt, _ptr(x), _ptr(dy), _ptr(addend), _ptr(dx), m, ih, iw, c, 1, st))
            return dx

        (h1, w1), (h2, w2), (h3, w3) = sizes[0], sizes[1], sizes[2]
        gk = dist[4]                                                       # at conv5's output
        gk = add(self._dgrad(4, m, h3, w3, gk, wd, x_act=f[3]), dist[3])  # at conv4's output
        gk = add(self._dgrad(3, m, h3, w3, gk, wd, x_act=f[2]), dist[2])  # at conv3's output
        gk = pool_bwd(f[1], self._dgrad(2, m, h3, w3, gk, wd), dist[1])   # through pool2 to conv2's output
        gk = pool_bwd(f[0], self._dgrad(1, m, h2, w2, gk, wd), dist[0])   # through pool1 to conv1's output
        gk = self._dgrad(0, m, h1 + 2, w1 + 2, gk, wd)                    # at the space-to-depth stem input
        if which & 1:
            check(lib.dsr_lpips_stem_prep_bwd(dt, _ptr(gk), n, h, w, int(self.normalize), float(scale), _ptr(out1), st))
        if which & 2:
            check(lib.dsr_lpips_stem_prep_bwd(dt, _ptr(gk[m - n:]), n, h, w, int(self.normalize), float(scale), _ptr(out2), st))


class _LPIPSFunction(torch.autograd.Function):
    """(per_image [N], total [1]) of LPIPS._run with the image gradients of LPIPS._trunk_bwd; the module's weights are
    constants of the node."""

    @staticmethod
    def forward(ctx, mod, img1, img2):
        chunks = []
        per, tot = mod._run(img1, img2, None, keep=chunks)
        ctx.mod, ctx.chunks = mod, chunks
        ctx.shape, ctx.dtypes = tuple(img1.shape), (img1.dtype, img2.dtype)
        ctx.set_materialize_grads(False)
        return per, tot

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, gtot):
        mod = ctx.mod
        n, _, h, w = ctx.shape
        which = (1 if ctx.needs_input_grad[1] else 0) | (2 if ctx.needs_input_grad[2] else 0)
        if which == 0 or (gper is None and gtot is None):
            return None, None, None
        dev = ctx.chunks[0][2][0].device
        sizes = mod.tap_sizes(h, w)
        g = mod._upstream(gper, gtot, n, dev)
        scale = mod._grad_scale(n, sizes)
        out = [torch.empty(ctx.shape, dtype=torch.float32, device=dev) if which & b else None for b in (1, 2)]
        for i0, i1, feats in ctx.chunks:
            mod._trunk_bwd(feats, i1 - i0, h, w, sizes, g[i0:i1], which, None if out[0] is None else out[0][i0:i1],
                           None if out[1] is None else out[1][i0:i1], scale)
        out = [o if o is None or o.dtype == dt else o.to(dt) for o, dt in zip(out, ctx.dtypes)]
        return None, out[0], out[1]
