"""The reference's data path (dataset.py:9-159) with the per-image arithmetic on the MI355X.

  get_image_pair / DIV2KDataset / GANDIV2KDataset   same names, constructor arguments and return values as the reference; file
        decoding stays Pillow on the host, everything after it (the bicubic resizes, the noise, ToTensor, scale_images, the
        training patches) runs as HIP kernels on device-resident uint8 images.  Items come back as device tensors.
  PatchBank   what the reference's DataLoader + GANDIV2KDataset amount to for a training step, restructured for the device: the
        whole (pre-shrunk) image set lives in HBM as uint8 and ``sample(batch)`` cuts and converts a batch of LR / HR patch
        pairs in two kernel launches -- the step is fed at its own rate instead of the host's; ``augment=True`` flips /
        turns each pair by a random element of D4 in the same launches; ``degradation=BlindDegradation(...)`` makes the LR
        patch from the HR image with a fresh blur kernel and noise level per sample (csrc/degrade.hip) and, with a
        ``jpeg_quality`` range, a JPEG round trip at a quality per sample after it (csrc/jpeg.hip).

The reference scales by 255 twice (ToTensor at :59-60, then scale_images :152,155): ``reference_scaling=True`` (default)
reproduces that, bit for bit; ``False`` gives the [0,1] / [-1,1] ranges its comments describe (SURVEY.md 8f row 1 asks for
the choice to be explicit).  torchvision is not needed (ToTensor = /255 into CHW float32).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .functional import _ptr, _stream, check
from .utils import degradation

PATCH_UNIT, PATCH_LR_REF, PATCH_HR_REF, PATCH_HR_UNIT = range(4)
BlindDegradation = degradation.BlindDegradation


def _device(device):
    return torch.device(device if device is not None else "cuda:0")


def _check_transforms(transforms, n, ph, pw):
    """The D4 codes of `n` ph x pw patches as ints: 0..7 each, and a quarter turn (odd code) only for a square patch."""
    codes = [int(k) for k in transforms]
    if len(codes) != n:
        raise ValueError(f"transforms: {len(codes)} codes for {n} patches")
    for k in codes:
        if not 0 <= k <= 7:
            raise ValueError(f"transforms: code {k} is not in 0..7")
        if k % 2 and ph != pw:
            raise ValueError(f"transforms: code {k} turns a {ph}x{pw} patch by a quarter; only 0, 2, 4, 6 keep its shape")
    return codes


def patch_batch(images, tops, lefts, ph, pw, mode, transforms=None):
    """fp32 [B,3,ph,pw] batch of patches, patch b cut from uint8 [H,W,3] device image images[b] at (tops[b], lefts[b]).
    ``transforms``: one D4 code per patch (0..7: k % 4 quarter turns of the patch, mirrored left-right first when k >= 4, as
    ``torch.rot90(torch.flip(x, [-1]) if k >= 4 else x, k % 4, [-2, -1])``), applied in the same launch."""
    n = len(images)
    if not (n == len(tops) == len(lefts)) or n == 0:
        raise ValueError("patch_batch: images, tops and lefts must be equally long and non-empty")
    codes = None if transforms is None else _check_transforms(transforms, n, ph, pw)
    for im in images:
        if not (torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
                and im.is_contiguous()):
            raise TypeError("patch_batch: images must be contiguous uint8 [H, W, 3] tensors on the device")
    out = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=images[0].device)
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
    ints = lambda v: (C.c_int * n)(*[int(q) for q in v])
    heights, widths = ints([im.shape[0] for im in images]), ints([im.shape[1] for im in images])
    if codes is None:
        check(_lib.lib().dsr_patch_batch_u8(n, ptrs, heights, widths, ints(tops), ints(lefts), ph, pw, mode, _ptr(out), _stream()))
    else:
        check(_lib.lib().dsr_patch_batch_u8_d4(n, ptrs, heights, widths, ints(tops), ints(lefts), ints(codes), ph, pw, mode,
                                               _ptr(out), _stream()))
    return out


def to_tensor(image):
    """uint8 [H,W,3] device image -> float32 [3,H,W] in [0,1] (torchvision ToTensor, dataset.py:59-60)."""
    return patch_batch([image.contiguous()], [0], [0], image.shape[0], image.shape[1], PATCH_UNIT)[0]


def get_image_pair(dataset_config, idx, device=None):
    """dataset.py:9-62.  Returns (LR [3,h,w], HR [3,H,W], filename): float32 device tensors in [0,1]."""
    from PIL import Image
    dev = _device(device if device is not None else getattr(dataset_config, "device", None))
    hr_path = os.path.join(dataset_config.HR_dir, dataset_config.HR_images[idx])
    filename, _ = os.path.splitext(dataset_config.HR_images[idx])
    lr_path = os.path.join(dataset_config.LR_dir, f"{filename}x8.png")
    up = lambda path: torch.from_numpy(np.array(Image.open(path).convert("RGB"))).to(dev)      # :12,19
    lr_u8, hr_u8 = _shrink_pair(up(lr_path), up(hr_path), dataset_config.scale_factor, dataset_config.downsample)
    nt = dataset_config.noise_type
    if nt is not None:                                                                         # :50-55
        if nt["type"] == "SaltAndPepper":
            lr_u8 = degradation.add_salt_pepper_noise(lr_u8, s=nt["s"], p=nt["p"])
        elif nt["type"] == "Gaussian":
            lr_u8 = degradation.add_gaussian_noise(lr_u8, std=nt["std"])
    return to_tensor(lr_u8), to_tensor(hr_u8), filename


def _shrink_pair(lr_u8, hr_u8, scale_factor, extra_downsample):
    """dataset.py:21-45 on device uint8 images: both halved, LR optionally halved again, HR resized to scale_factor x LR (the
    `and` of :35 is kept as written)."""
    lr_u8 = degradation.downsample(lr_u8, 2)
    hr_u8 = degradation.downsample(hr_u8, 2)
    if extra_downsample:
        lr_u8 = degradation.downsample(lr_u8)
    h_lr, w_lr = lr_u8.shape[0], lr_u8.shape[1]
    w_hr, h_hr = scale_factor * w_lr, scale_factor * h_lr
    if w_hr > hr_u8.shape[1] and h_hr > hr_u8.shape[0]:
        w_hr = (hr_u8.shape[1] // scale_factor) * scale_factor
        h_hr = (hr_u8.shape[0] // scale_factor) * scale_factor
        w_lr, h_lr = w_hr // scale_factor, h_hr // scale_factor
        hr_u8 = degradation.resize(hr_u8, w_hr, h_hr)
        lr_u8 = degradation.resize(lr_u8, w_lr, h_lr)
    else:
        hr_u8 = degradation.resize(hr_u8, w_hr, h_hr)
    return lr_u8, hr_u8


class DIV2KDataset(torch.utils.data.Dataset):
    """dataset.py:68-95."""

    def __init__(self, LR_dir, scale_factor, downsample=False, noise_type=None, num_images=-1, HR_dir=None, device=None):
        super().__init__()
        self.downsample, self.noise_type, self.scale_factor = downsample, noise_type, scale_factor
        self.LR_dir, self.HR_dir, self.device = LR_dir, HR_dir, device
        self.LR_images, self.HR_images = os.listdir(LR_dir), os.listdir(HR_dir)
        if num_images > 0:
            self.LR_images, self.HR_images = self.LR_images[:num_images], self.HR_images[:num_images]

    def __getitem__(self, idx):
        return get_image_pair(self, idx)

    def __len__(self):
        return len(self.LR_images)


class GANDIV2KDataset(torch.utils.data.Dataset):
    """dataset.py:98-171."""

    def __init__(self, LR_dir, scale_factor, downsample=False, noise_type=None, num_images=-1, HR_dir=None, LR_patch_size=None,
                 train=False, device=None):
        super().__init__()
        self.train = train
        self.downsample, self.noise_type, self.scale_factor = downsample, noise_type, scale_factor
        self.LR_dir, self.HR_dir, self.device = LR_dir, HR_dir, device
        self.LR_images, self.HR_images = os.listdir(LR_dir), os.listdir(HR_dir)
        if num_images > 0:
            self.LR_images, self.HR_images = self.LR_images[:num_images], self.HR_images[:num_images]
        self.LR_patch_size = LR_patch_size

    def get_train_patches(self, LR_image, HR_image):
        """dataset.py:121-147 (the two randint draws from numpy's global generator, x first): views into the CHW tensors."""
        _, lr_h, lr_w = LR_image.size()
        top, left, hr_top, hr_left = train_patch_coords(lr_h, lr_w, self.LR_patch_size, self.scale_factor)
        pw, ph = self.LR_patch_size
        s = self.scale_factor
        return (LR_image[:, top:top + ph, left:left + pw], HR_image[:, hr_top:hr_top + ph * s, hr_left:hr_left + pw * s])

    @staticmethod
    def scale_images(LR_image, HR_image):
        """dataset.py:149-159 as written (in place): LR /= 255; HR = HR / 255 * 2 - 1, on tensors ToTensor already put in [0,1].
        On the HIP kernel dsr_scale_images_f32: ATen's device `x /= 255.0` multiplies by the reciprocal, one ulp off the host."""
        for t, mode in ((LR_image, PATCH_LR_REF), (HR_image, PATCH_HR_REF)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise TypeError("scale_images: contiguous float32 device tensors expected")
            check(_lib.lib().dsr_scale_images_f32(_ptr(t), t.numel(), mode, _stream()))
        return LR_image, HR_image

    def __getitem__(self, idx):
        LR_image, HR_image, filename = get_image_pair(self, idx)
        LR_image, HR_image = GANDIV2KDataset.scale_images(LR_image, HR_image)
        if self.train:
            LR_image, HR_image = self.get_train_patches(LR_image, HR_image)
        return LR_image, HR_image, filename

    def __len__(self):
        return len(self.LR_images)


def train_patch_coords(lr_h, lr_w, LR_patch_size, scale_factor, rng=None):
    """(LR top, LR left, HR top, HR left) of dataset.py:121-141; `rng` defaults to numpy's global generator like the reference."""
    rng = np.random if rng is None else rng
    pw, ph = LR_patch_size
    cx = rng.randint(pw // 2, lr_w - pw // 2)
    cy = rng.randint(ph // 2, lr_h - ph // 2)
    left, top = int(cx - pw // 2), int(cy - ph // 2)
    return top, left, top * scale_factor, left * scale_factor


class PatchBank:
    """A (pre-shrunk, optionally degraded) image set resident in HBM as uint8, and batches of training patches cut from it on
    the device: ``sample(batch)`` = `batch` draws of (image index, patch position) + two launches of dsr_patch_batch_u8.

    pairs: iterable of (LR uint8 [h,w,3], HR uint8 [h*s, w*s, 3]) device tensors (e.g. from `_shrink_pair` + degradations).
    augment: every sample is flipped / turned by one of the eight D4 codes (`patch_batch`), the same for its LR and its HR
        patch, in the launches that cut them (dsr_patch_batch_u8_d4).  The codes are drawn AFTER all indices and positions, so
        a seeded bank crops the same patches with and without augmentation; a non-square patch only gets the four codes that
        keep its shape.
    degradation: a `BlindDegradation`.  The LR patch is then cut from the HR image by dsr_degrade_batch_u8 with a fresh blur
        kernel (and noise level) per sample: ``LR = quant(clip((HR (*) k)[offset::s, offset::s] + sigma * z))``.  The LR image
        of a pair only supplies the size of the LR grid and may be None (the grid is then HR // s); the HR patch comes from
        the same launch as without it.  The kernels and noise levels are drawn AFTER the indices, positions and D4 codes (a
        seeded bank crops the same patches, with the same codes, with and without `degradation`): the kernels by
        ``degradation.random_kernels`` (four uniform draws per sample), then, only if the noise range is not (0, 0), `batch`
        uniform noise levels.  The noise itself is ``torch.randn`` on the device (`generator`).  ``last_kernels`` /
        ``last_noise_std`` hold the device tensors of the values used, e.g. as targets of a kernel estimator.
        With ``degradation.jpeg_quality = (low, high)`` the degraded patch finishes with a JPEG round trip (BSRGAN,
        Real-ESRGAN): it is cut in PATCH_UNIT scaling and rounded to whole grey levels whatever `quantise` says, passed
        through ``degradation.jpeg_batch`` at a quality per sample and leaves in the bank's LR scaling.  The patch is the
        image: the 8x8 grid starts at its corner, after the D4 code.  The qualities are drawn LAST, `batch` draws of
        ``rng.randint(low, high + 1)``, and only with a range; ``last_jpeg_quality`` is the int32 device tensor used."""

    def __init__(self, pairs, scale_factor, LR_patch_size, reference_scaling=True, rng=None, augment=False, degradation=None,
                 generator=None):
        pairs = list(pairs)
        if not pairs:
            raise ValueError("PatchBank needs at least one image pair")
        if degradation is not None:
            degradation.validate(scale_factor)
        elif any(p[0] is None for p in pairs):
            raise ValueError("a pair without an LR image needs a `degradation` that makes one")
        self.lr = [None if p[0] is None else p[0].contiguous() for p in pairs]
        self.hr = [p[1].contiguous() for p in pairs]
        # (h, w) of each LR grid: what the patch positions are drawn in
        self.grid = [(b.shape[0] // scale_factor, b.shape[1] // scale_factor) if a is None else (a.shape[0], a.shape[1])
                     for a, b in zip(self.lr, self.hr)]
        for (h, w), b in zip(self.grid, self.hr):
            if b.shape[0] < h * scale_factor or b.shape[1] < w * scale_factor:
                raise ValueError("an HR image is smaller than scale_factor x its LR image")
        self.scale, self.patch = scale_factor, tuple(LR_patch_size)
        self.modes = (PATCH_LR_REF, PATCH_HR_REF) if reference_scaling else (PATCH_UNIT, PATCH_HR_UNIT)
        self.rng = np.random if rng is None else rng
        self.augment = bool(augment)
        self.degradation, self.generator = degradation, generator
        self.last_kernels = self.last_noise_std = self.last_jpeg_quality = None

    @classmethod
    def from_hr(cls, hr_images, scale_factor, LR_patch_size, **kw):
        """A bank built from HR images alone, the way the benchmark LR sets were built: each uint8 [H, W, 3] HR image (device
        tensor or numpy array) is cropped to a multiple of `scale_factor` (``modcrop``) and its LR image is made once, on the
        device, by the MATLAB-style ``utils.imresize.imresize(hr, 1 / scale_factor)`` (bicubic, antialiased).  `kw`: the
        constructor's other arguments."""
        from .utils.imresize import imresize, modcrop
        dev = None
        pairs = []
        for hr in hr_images:
            if not torch.is_tensor(hr):
                hr = torch.from_numpy(np.ascontiguousarray(hr)).to(_device(dev))
            dev = hr.device
            hr = modcrop(hr, scale_factor).contiguous()
            pairs.append((imresize(hr, scale=1.0 / scale_factor), hr))
        return cls(pairs, scale_factor, LR_patch_size, **kw)

    def sample(self, batch, indices=None, transforms=None, kernels=None, noise_std=None, jpeg_quality=None):
        """(LR [B,3,ph,pw], HR [B,3,ph*s,pw*s]) fp32 device batches; image b is `indices[b]` (default: uniform draws).
        ``transforms``: explicit D4 codes, one per sample, instead of the draw (also without ``augment``).
        ``kernels`` (fp32 [B, ks, ks], numpy or tensor) / ``noise_std`` ([B], 0..255 units): explicit blur kernels / noise
        levels instead of the draws of a bank with a ``degradation``; ``jpeg_quality`` ([B] integers in 1..100): explicit
        JPEG qualities instead of the draws of a degradation with a ``jpeg_quality`` range."""
        pw, ph = self.patch
        n = batch if indices is None else len(indices)
        if transforms is not None:
            transforms = _check_transforms(transforms, n, ph, pw)
        deg = self.degradation
        if deg is None and (kernels is not None or noise_std is not None):
            raise ValueError("kernels / noise_std need a bank with a `degradation`")
        if kernels is not None:
            shape = tuple(kernels.shape)
            if len(shape) != 3 or shape[0] != n or shape[1] != shape[2] or shape[1] % 2 == 0 or shape[1] > degradation.KERNEL_SIZE_MAX:
                raise ValueError(f"kernels: {shape} is not [{n}, ks, ks] with an odd ks <= {degradation.KERNEL_SIZE_MAX}")
        if noise_std is not None:
            noise_std = np.asarray(noise_std.cpu() if torch.is_tensor(noise_std) else noise_std, dtype=np.float32).reshape(-1)
            if noise_std.shape[0] != n or bool((noise_std < 0).any()):
                raise ValueError(f"noise_std: {n} non-negative levels expected")
        if jpeg_quality is not None:
            if deg is None or deg.jpeg_quality is None:
                raise ValueError("jpeg_quality needs a bank whose `degradation` has a jpeg_quality range")
            jpeg_quality = [int(q) if degradation._is_int(q) else q
                            for q in (jpeg_quality.tolist() if hasattr(jpeg_quality, "tolist") else jpeg_quality)]
            if len(jpeg_quality) != n or not all(degradation._is_int(q) and 1 <= q <= 100 for q in jpeg_quality):
                raise ValueError(f"jpeg_quality: {n} integers in 1..100 expected")
        if indices is None:
            indices = [int(self.rng.randint(0, len(self.hr))) for _ in range(batch)]
        tops, lefts, htops, hlefts = [], [], [], []
        for i in indices:
            t, l, ht, hl = train_patch_coords(self.grid[i][0], self.grid[i][1], self.patch, self.scale, self.rng)
            tops.append(t), lefts.append(l), htops.append(ht), hlefts.append(hl)
        if transforms is None and self.augment:
            if ph == pw:
                transforms = [int(self.rng.randint(0, 8)) for _ in indices]
            else:
                transforms = [2 * int(self.rng.randint(0, 4)) for _ in indices]
        if deg is None:
            lr = patch_batch([self.lr[i] for i in indices], tops, lefts, ph, pw, self.modes[0], transforms)
        else:
            lr = self._degraded(deg, indices, tops, lefts, transforms, kernels, noise_std, jpeg_quality)
        hr = patch_batch([self.hr[i] for i in indices], htops, hlefts, ph * self.scale, pw * self.scale, self.modes[1], transforms)
        return lr, hr

    def _degraded(self, deg, indices, tops, lefts, transforms, kernels, noise_std, jpeg_quality=None):
        pw, ph = self.patch
        n = len(indices)
        dev = self.hr[0].device
        if kernels is None:
            kernels = degradation.random_kernels(n, deg.kernel_size, deg.sigma, deg.iso_prob, self.rng)
        if noise_std is None and deg.noise_std[1] > 0:
            noise_std = np.asarray(self.rng.uniform(deg.noise_std[0], deg.noise_std[1], n), dtype=np.float32)
        if isinstance(kernels, np.ndarray):
            kernels = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float32))
        self.last_kernels = kernels.to(device=dev, dtype=torch.float32).contiguous()            # one transfer
        z = None
        self.last_noise_std = None
        if noise_std is not None:
            self.last_noise_std = torch.from_numpy(noise_std).to(dev)                           # one transfer
            z = torch.randn((n, 3, ph, pw), dtype=torch.float32, device=dev, generator=self.generator)
        self.last_jpeg_quality = None
        if deg.jpeg_quality is None:
            return degradation.degrade_batch([self.hr[i] for i in indices], tops, lefts, ph, pw, self.scale, self.last_kernels,
                                             offset=deg.offset, noise=z, noise_std=self.last_noise_std, quantise=deg.quantise,
                                             mode=self.modes[0], transforms=transforms)
        if jpeg_quality is None:
            jpeg_quality = [int(self.rng.randint(deg.jpeg_quality[0], deg.jpeg_quality[1] + 1)) for _ in range(n)]
        self.last_jpeg_quality = torch.tensor(jpeg_quality, dtype=torch.int32).to(dev)           # one transfer
        lr = degradation.degrade_batch([self.hr[i] for i in indices], tops, lefts, ph, pw, self.scale, self.last_kernels,
                                       offset=deg.offset, noise=z, noise_std=self.last_noise_std, quantise=True,
                                       mode=PATCH_UNIT, transforms=transforms)
        return degradation.jpeg_batch(lr, self.last_jpeg_quality, deg.jpeg_subsampling, self.modes[0])
