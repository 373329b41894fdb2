"""The reference's degradations (utils/degradation.py:5-20) on device-resident uint8 images, computed by HIP kernels.

Same function names and argument meaning as the reference; an image here is a ``torch.uint8`` tensor ``[H, W, 3]`` on the
MI355X (what ``np.array(PIL image)`` holds on the host).  Numpy arrays and PIL images are accepted too -- they are uploaded,
processed on the device and returned in the type they came in -- so the reference's call sites keep working.

Bit-exactness: ``downsample`` reproduces Pillow's 8-bit bicubic resampler (fixed-point tables built here exactly like
libImaging/Resample.c's precompute_coeffs, the two passes run in csrc/data.hip); the noise functions draw from numpy's global
generator in the reference's order by default (``rng="numpy"``: same pixels as the reference for the same seed) or on the
device (``rng="device"``: torch's generator, for throughput).

Beyond the reference, the blind degradation of SRMD / IKC / KernelGAN / BSRGAN (csrc/degrade.hip):
``LR = quant(clip((HR (*) k)[offset::s, offset::s] + sigma * z))`` with a blur kernel per sample -- ``gaussian_kernel`` and
``random_kernels`` make the kernels on the host, ``blur_downsample`` degrades a whole image to uint8 and ``degrade_batch``
cuts a batch of degraded LR patches straight out of HR images (``dataset.PatchBank(degradation=...)`` is built on it).
The last stage of the BSRGAN / Real-ESRGAN recipe is a JPEG round trip at a random quality (csrc/jpeg.hip): ``jpeg_compress``
on uint8 images and ``jpeg_batch`` on fp32 patch batches, equal to Pillow's encoder and decoder bit for bit.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..functional import _need_gpu, _ptr, _stream, check

PRECISION_BITS = 32 - 8 - 2
_tables = {}


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_tables(in_size, out_size, device):
    """(ksize, bounds int32 [out][2], kk int32 [out][ksize]) of Pillow's bicubic resampler for one axis, on `device` (cached).
    Host float64 arithmetic in Pillow's order (precompute_coeffs, normalize_coeffs_8bpc); uploaded once per (in, out)."""
    key = (in_size, out_size, str(device))
    hit = _tables.get(key)
    if hit is not None:
        return hit
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * inv) for x in range(xmax)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            if total != 0.0:
                v = v / total
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    out = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device))
    _tables[key] = out
    return out


def _to_device(image, device=None):
    """-> (uint8 [H,W,C] device tensor, restore(tensor) -> the caller's type)."""
    if torch.is_tensor(image):
        _need_gpu(image)
        if image.dtype != torch.uint8 or image.dim() != 3:
            raise TypeError(f"image tensor must be uint8 [H, W, C], got {image.dtype} {tuple(image.shape)}")
        return image.contiguous(), (lambda t: t)
    dev = torch.device(device if device is not None else "cuda:0")
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8 or image.ndim != 3:
            raise TypeError(f"image array must be uint8 [H, W, C], got {image.dtype} {image.shape}")
        return torch.from_numpy(np.ascontiguousarray(image)).to(dev), (lambda t: t.cpu().numpy())
    from PIL import Image                                            # a PIL image (what the reference's downsample takes)
    arr = np.array(image.convert("RGB"))
    return torch.from_numpy(arr).to(dev), (lambda t: Image.fromarray(t.cpu().numpy()))


def resize(image, out_w, out_h):
    """``PIL.Image.resize((out_w, out_h), Image.BICUBIC)`` (dataset.py:38-45) on the device."""
    img, restore = _to_device(image)
    h, w, c = img.shape
    lib = _lib.lib()
    out = img
    if out_w != w:
        ksize, bounds, kk = resample_tables(w, out_w, img.device)
        dst = torch.empty((h, out_w, c), dtype=torch.uint8, device=img.device)
        check(lib.dsr_resample_u8(_ptr(out), _ptr(dst), h, w, c, 1, out_w, _ptr(bounds), _ptr(kk), ksize, _stream()))
        out = dst
    if out_h != h:
        ksize, bounds, kk = resample_tables(h, out_h, img.device)
        dst = torch.empty((out_h, out.shape[1], c), dtype=torch.uint8, device=img.device)
        check(lib.dsr_resample_u8(_ptr(out), _ptr(dst), h, out.shape[1], c, 0, out_h, _ptr(bounds), _ptr(kk), ksize, _stream()))
        out = dst
    return restore(out)


def downsample(image, factor=2, interpolation=None):
    """utils/degradation.py:19-20: bicubic resize to (W // factor, H // factor).  `interpolation` other than bicubic is refused
    (the reference only ever passes its default)."""
    if interpolation is not None:
        from PIL import Image
        if interpolation != Image.BICUBIC:
            raise NotImplementedError("only Image.BICUBIC (the reference's default) is implemented on the device")
    if torch.is_tensor(image) or isinstance(image, np.ndarray):
        h, w = image.shape[0], image.shape[1]
    else:
        w, h = image.width, image.height
    return resize(image, w // factor, h // factor)


def add_gaussian_noise(image, std=1, rng="numpy"):
    """utils/degradation.py:5-7: clip(image + N(0, (std*255)^2), 0, 255) truncated to uint8.  rng="numpy": the normal draw comes
    from numpy's global generator (float64, same call as the reference: same result for the same seed); "device": torch."""
    img, restore = _to_device(image)
    if rng == "numpy":
        noise = torch.from_numpy(np.random.normal(scale=std * 255, size=tuple(img.shape))).to(img.device)   # float64
    elif rng == "device":
        noise = torch.randn(tuple(img.shape), dtype=torch.float32, device=img.device) * float(std * 255)
    else:
        raise ValueError("rng must be 'numpy' or 'device'")
    out = torch.empty_like(img)
    check(_lib.lib().dsr_noise_gaussian_u8(_ptr(img), _ptr(noise), int(noise.dtype == torch.float64), _ptr(out), img.numel(),
                                           _stream()))
    return restore(out)


def add_salt_pepper_noise(image, s=0.01, p=0.01, rng="numpy"):
    """utils/degradation.py:9-17: salt (255) where rand < s, then pepper (0) where rand < p, per pixel over all channels.
    Returns a new image (the reference writes into its argument and returns it)."""
    img, restore = _to_device(image)
    h, w, c = img.shape
    if rng == "numpy":
        salt = torch.from_numpy(np.random.rand(h, w) < s).to(img.device)
        pepper = torch.from_numpy(np.random.rand(h, w) < p).to(img.device)
    elif rng == "device":
        salt = torch.rand((h, w), device=img.device) < s
        pepper = torch.rand((h, w), device=img.device) < p
    else:
        raise ValueError("rng must be 'numpy' or 'device'")
    salt, pepper = salt.to(torch.uint8).contiguous(), pepper.to(torch.uint8).contiguous()
    out = torch.empty_like(img)
    check(_lib.lib().dsr_salt_pepper_u8(_ptr(img), _ptr(salt), _ptr(pepper), _ptr(out), h, w, c, _stream()))
    return restore(out)


# ------------------------------------------------------------------ blind degradation (csrc/degrade.hip)
KERNEL_SIZE_MAX = 21


def gaussian_kernel(size, sigma_x, sigma_y=None, theta=0.0):
    """fp32 [size, size] bivariate Gaussian with covariance R diag(sigma_x^2, sigma_y^2) R^T (R: rotation by `theta`),
    evaluated in float64 at (x, y) = (j - r, i - r), r = size // 2, normalised to sum 1 and rounded to fp32 once.
    ``sigma_y=None``: isotropic."""
    size = int(size)
    if size < 1 or size % 2 == 0:
        raise ValueError(f"gaussian_kernel: size {size} is not a positive odd number")
    sigma_y = sigma_x if sigma_y is None else sigma_y
    if not (sigma_x > 0 and sigma_y > 0):
        raise ValueError("gaussian_kernel: sigmas must be positive")
    r = size // 2
    y, x = np.meshgrid(np.arange(size, dtype=np.float64) - r, np.arange(size, dtype=np.float64) - r, indexing="ij")
    c, sn = math.cos(theta), math.sin(theta)
    u, v = c * x + sn * y, -sn * x + c * y                          # R^T (x, y): the coordinates along the two axes
    k = np.exp(-0.5 * (u * u / (float(sigma_x) ** 2) + v * v / (float(sigma_y) ** 2)))
    return (k / k.sum()).astype(np.float32)


def random_kernels(n, size=21, sigma=(0.2, 3.0), iso_prob=0.5, rng=None):
    """fp32 [n, size, size] random Gaussian blur kernels on the host.  Per sample, in this order, four ``rng.uniform`` draws:
    u in [0, 1) (isotropic iff u < iso_prob), sigma_x and sigma_y in [sigma[0], sigma[1]), theta in [-pi, pi).  All four are
    always drawn; an isotropic sample uses sigma_x alone.  `rng` defaults to numpy's global generator."""
    rng = np.random if rng is None else rng
    lo, hi = float(sigma[0]), float(sigma[1])
    if not 0 < lo <= hi:
        raise ValueError(f"random_kernels: sigma range ({lo}, {hi}) is not 0 < low <= high")
    out = np.empty((n, size, size), dtype=np.float32)
    for b in range(n):
        iso = float(rng.uniform(0.0, 1.0)) < iso_prob
        sx = float(rng.uniform(lo, hi))
        sy = float(rng.uniform(lo, hi))
        theta = float(rng.uniform(-math.pi, math.pi))
        out[b] = gaussian_kernel(size, sx) if iso else gaussian_kernel(size, sx, sy, theta)
    return out


def _device_kernels(kernels, n, device):
    """-> contiguous fp32 [n, ks, ks] on `device` (one upload when the kernels come from the host)"""
    k = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float32)) if isinstance(kernels, np.ndarray) else kernels
    if not torch.is_tensor(k) or k.dtype != torch.float32 or k.dim() != 3 or k.shape[0] != n or k.shape[1] != k.shape[2]:
        raise ValueError(f"kernels must be fp32 [{n}, ks, ks]")
    ks = int(k.shape[1])
    if ks % 2 == 0 or ks > KERNEL_SIZE_MAX:
        raise ValueError(f"kernel size {ks} is not an odd number in 1..{KERNEL_SIZE_MAX}")
    return k.to(device).contiguous(), ks


def blur_downsample(image, kernel, factor, offset=0, noise_std=0.0, generator=None):
    """uint8 [H, W, 3] -> uint8 [h, w, 3], h = ceil((H - offset) / factor): the image blurred with `kernel` (fp32 [ks, ks],
    reflected borders), sampled at ``[offset::factor, offset::factor]``, plus ``noise_std`` (0..255 units) times a standard
    normal drawn on the device (only when noise_std > 0; `generator`: a torch.Generator), clipped and rounded half to even.
    The image may be a device tensor, a numpy array or a PIL image and comes back in that type."""
    img, restore = _to_device(image)
    if img.shape[2] != 3:
        raise TypeError("blur_downsample: an RGB image [H, W, 3] is expected")
    k, ks = _device_kernels(kernel[None] if getattr(kernel, "ndim", 0) == 2 else kernel, 1, img.device)
    H, W = int(img.shape[0]), int(img.shape[1])
    factor, offset = int(factor), int(offset)
    if factor < 1 or not 0 <= offset < factor:
        raise ValueError(f"blur_downsample: factor {factor}, offset {offset}")
    h, w = (H - offset + factor - 1) // factor, (W - offset + factor - 1) // factor
    z = std = None
    if noise_std > 0:
        z = torch.randn((3, h, w), dtype=torch.float32, device=img.device, generator=generator)
        std = torch.full((1,), float(noise_std), dtype=torch.float32, device=img.device)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
    check(_lib.lib().dsr_degrade_image_u8(_ptr(img), H, W, factor, offset, _ptr(k), ks, None if z is None else _ptr(z),
                                          None if std is None else _ptr(std), _ptr(out), _stream()))
    return restore(out)


def degrade_batch(images, tops, lefts, ph, pw, scale, kernels, offset=0, noise=None, noise_std=None, quantise=True, mode=0,
                  transforms=None):
    """fp32 [B, 3, ph, pw] batch of degraded LR patches, patch b cut from the uint8 [H, W, 3] HR device image images[b] at the
    LR position (tops[b], lefts[b]): the counterpart of ``dataset.patch_batch`` (same `mode` and `transforms`), one launch of
    dsr_degrade_batch_u8.  kernels: fp32 [B, ks, ks] (device tensor, or numpy: uploaded once); noise: device fp32 [B, 3, ph, pw]
    standard-normal draws with noise_std: fp32 [B] in 0..255 units (device tensor or a sequence), both or neither."""
    from ..dataset import _check_transforms
    n = len(images)
    if not (n == len(tops) == len(lefts)) or n == 0:
        raise ValueError("degrade_batch: images, tops and lefts must be equally long and non-empty")
    codes = None if transforms is None else _check_transforms(transforms, n, ph, pw)
    if (noise is None) != (noise_std is None):
        raise ValueError("degrade_batch: noise and noise_std go together")
    for im in images:
        if not (torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
                and im.is_contiguous()):
            raise TypeError("degrade_batch: images must be contiguous uint8 [H, W, 3] tensors on the device")
    dev = images[0].device
    k, ks = _device_kernels(kernels, n, dev)
    if noise is not None:
        if not (torch.is_tensor(noise) and noise.dtype == torch.float32 and tuple(noise.shape) == (n, 3, ph, pw)):
            raise ValueError(f"degrade_batch: noise must be fp32 [{n}, 3, {ph}, {pw}]")
        noise = noise.to(dev).contiguous()
        if not torch.is_tensor(noise_std):
            noise_std = torch.tensor([float(v) for v in noise_std], dtype=torch.float32)
        if noise_std.dtype != torch.float32 or tuple(noise_std.shape) != (n,):
            raise ValueError(f"degrade_batch: noise_std must be fp32 [{n}]")
        noise_std = noise_std.to(dev).contiguous()
    out = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
    ints = lambda v: (C.c_int * n)(*[int(q) for q in v])
    check(_lib.lib().dsr_degrade_batch_u8(n, ptrs, ints([im.shape[0] for im in images]), ints([im.shape[1] for im in images]),
                                          ints(tops), ints(lefts), None if codes is None else ints(codes), ph, pw, int(scale),
                                          int(offset), _ptr(k), ks, None if noise is None else _ptr(noise),
                                          None if noise is None else _ptr(noise_std), int(bool(quantise)), int(mode), _ptr(out),
                                          _stream()))
    return out


# ------------------------------------------------------------------ JPEG round trip (csrc/jpeg.hip)
def _subsampling(subsampling):
    """"4:4:4" / 0 -> 0, "4:2:0" / 2 -> 2 (Pillow's numbers); anything else is refused"""
    if isinstance(subsampling, str):
        if subsampling in ("4:4:4", "4:2:0"):
            return 0 if subsampling == "4:4:4" else 2
    elif not isinstance(subsampling, bool) and subsampling in (0, 2):
        return int(subsampling)
    raise ValueError(f"subsampling {subsampling!r} is not '4:4:4' / 0 or '4:2:0' / 2")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _device_qualities(quality, n, device):
    """-> int32 [n] on `device`.  An int (for every sample), a sequence, numpy array or host tensor of n integers: checked to
    lie in 1..100 and uploaded once.  An int32 device tensor [n] is used as it is, with no host read (the kernels clamp)."""
    if torch.is_tensor(quality) and quality.is_cuda:
        if quality.dtype != torch.int32 or tuple(quality.shape) != (n,):
            raise ValueError(f"quality: a device tensor must be int32 [{n}], got {quality.dtype} {tuple(quality.shape)}")
        return quality.to(device).contiguous()
    if torch.is_tensor(quality):
        if quality.dtype.is_floating_point or quality.dtype == torch.bool:
            raise ValueError(f"quality: integers are expected, got {quality.dtype}")
        quality = quality.reshape(-1).tolist()
    elif isinstance(quality, np.ndarray):
        if not np.issubdtype(quality.dtype, np.integer):
            raise ValueError(f"quality: integers are expected, got {quality.dtype}")
        quality = quality.reshape(-1).tolist()
    elif _is_int(quality):
        quality = [quality] * n
    else:
        try:
            quality = list(quality)
        except TypeError:
            raise ValueError(f"quality {quality!r} is neither an integer nor a sequence of integers") from None
    if len(quality) != n:
        raise ValueError(f"quality: {len(quality)} values for {n} images")
    for q in quality:
        if not _is_int(q) or not 1 <= q <= 100:
            raise ValueError(f"quality {q!r} is not an integer in 1..100")
    return torch.tensor([int(q) for q in quality], dtype=torch.int32).to(device)


def _jpeg_workspace(lib, n, h, w, ss, device):
    size = lib.dsr_jpeg_workspace(n, h, w, ss)
    return None if size == 0 else torch.empty((size,), dtype=torch.uint8, device=device)


def jpeg_compress(image, quality=75, subsampling="4:2:0"):
    """What ``PIL.Image.save(f, 'JPEG', quality=quality, subsampling=...)`` followed by ``Image.open(f)`` does to a uint8 RGB
    image, bit for bit, on the device (dsr_jpeg_u8; no bitstream is made).  image: [H, W, 3] as a device tensor, a numpy
    array or a PIL image, returned in that type; or a device tensor [B, H, W, 3] with one quality for all or one per image
    (a sequence, or an int32 device tensor, which is not read back).  subsampling: "4:4:4" / 0 or "4:2:0" / 2."""
    ss = _subsampling(subsampling)
    if torch.is_tensor(image) and image.dim() == 4:
        _need_gpu(image)
        if image.dtype != torch.uint8:
            raise TypeError(f"image tensor must be uint8, got {image.dtype}")
        img, restore = image.contiguous(), (lambda t: t)
    else:
        img, restore = _to_device(image)
        img = img[None]
    if img.shape[3] != 3 or img.shape[0] == 0 or img.shape[1] == 0 or img.shape[2] == 0:
        raise TypeError(f"jpeg_compress: RGB images [H, W, 3] or [B, H, W, 3] are expected, got {tuple(image.shape)}")
    n, h, w = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
    q = _device_qualities(quality, n, img.device)
    lib = _lib.lib()
    ws = _jpeg_workspace(lib, n, h, w, ss, img.device)
    out = torch.empty_like(img)
    check(lib.dsr_jpeg_u8(_ptr(img), _ptr(out), n, h, w, _ptr(q), ss, None if ws is None else _ptr(ws), _stream()))
    return restore(out if torch.is_tensor(image) and image.dim() == 4 else out[0])


def jpeg_batch(x, quality, subsampling="4:2:0", mode=0):
    """fp32 [B, 3, h, w] device batch in PATCH_UNIT scaling ([0, 1]) -> the batch after a JPEG round trip of its grey levels
    ``rint(clip(255 x, 0, 255))``, scaled by `mode` as ``dataset.patch_batch`` scales (dsr_jpeg_batch_f32; a new tensor).
    quality: as ``jpeg_compress``.  Every image is its own JPEG: the 8x8 grid starts at its corner."""
    ss = _subsampling(subsampling)
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.numel() > 0):
        raise TypeError("jpeg_batch: an fp32 [B, 3, h, w] tensor is expected")
    _need_gpu(x)
    if not _is_int(mode) or not 0 <= mode <= 3:
        raise ValueError(f"jpeg_batch: mode {mode!r} is not one of the four patch scalings 0..3")
    x = x.contiguous()
    n, h, w = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    q = _device_qualities(quality, n, x.device)
    lib = _lib.lib()
    ws = _jpeg_workspace(lib, n, h, w, ss, x.device)
    out = torch.empty_like(x)
    check(lib.dsr_jpeg_batch_f32(_ptr(x), _ptr(out), n, h, w, _ptr(q), ss, int(mode), None if ws is None else _ptr(ws), _stream()))
    return out


class BlindDegradation:
    """What ``dataset.PatchBank(degradation=...)`` draws per sample: a Gaussian blur kernel of `kernel_size` as
    ``random_kernels(sigma=, iso_prob=)`` and a noise level, uniform in `noise_std` = (low, high) in 0..255 units (no noise
    when high is 0); `quantise`: round the LR patch to whole grey levels; `offset`: the sampling phase in 0..scale-1.
    `jpeg_quality` = (low, high), integers in 1..100, both included: the degraded patch then goes through a JPEG round trip
    (``jpeg_batch``, chroma `jpeg_subsampling`) at a quality drawn per sample; None: no JPEG stage."""

    def __init__(self, kernel_size=21, sigma=(0.2, 3.0), iso_prob=0.5, noise_std=(0.0, 0.0), quantise=True, offset=0,
                 jpeg_quality=None, jpeg_subsampling="4:2:0"):
        self.kernel_size, self.sigma, self.iso_prob = int(kernel_size), (float(sigma[0]), float(sigma[1])), float(iso_prob)
        self.noise_std, self.quantise, self.offset = (float(noise_std[0]), float(noise_std[1])), bool(quantise), int(offset)
        self.jpeg_quality = None if jpeg_quality is None else tuple(jpeg_quality)
        self.jpeg_subsampling = jpeg_subsampling

    def validate(self, scale):
        if self.kernel_size < 1 or self.kernel_size % 2 == 0 or self.kernel_size > KERNEL_SIZE_MAX:
            raise ValueError(f"BlindDegradation: kernel_size {self.kernel_size} is not an odd number in 1..{KERNEL_SIZE_MAX}")
        if not 0 < self.sigma[0] <= self.sigma[1]:
            raise ValueError(f"BlindDegradation: sigma range {self.sigma} is not 0 < low <= high")
        if not 0.0 <= self.iso_prob <= 1.0:
            raise ValueError(f"BlindDegradation: iso_prob {self.iso_prob}")
        if not 0.0 <= self.noise_std[0] <= self.noise_std[1]:
            raise ValueError(f"BlindDegradation: noise_std range {self.noise_std} is not 0 <= low <= high")
        if not 0 <= self.offset < scale:
            raise ValueError(f"BlindDegradation: offset {self.offset} is not in 0..{scale - 1}")
        if self.jpeg_quality is not None:
            q = self.jpeg_quality
            if len(q) != 2 or not all(_is_int(v) for v in q) or not 1 <= q[0] <= q[1] <= 100:
                raise ValueError(f"BlindDegradation: jpeg_quality {q} is not (low, high) with integers 1 <= low <= high <= 100")
        _subsampling(self.jpeg_subsampling)
