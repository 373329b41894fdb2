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


def _rotated_q(size, sigma_x, sigma_y, theta, who):
    """u^2 / sigma_x^2 + v^2 / sigma_y^2 on the grid of ``gaussian_kernel``, with its statements"""
    size = int(size)
    if size < 1 or size % 2 == 0:
        raise ValueError(f"{who}: size {size} is not a positive odd number")
    sigma_y = sigma_x if sigma_y is None else sigma_y
    if not (sigma_x > 0 and sigma_y > 0):
        raise ValueError(f"{who}: sigmas must be positive")
    r = size // 2
    y, x = np.meshgrid(np.arange(size, dtype=np.float64) - r, np.arange(size, dtype=np.float64) - r, indexing="ij")
    c, sn = math.cos(theta), math.sin(theta)
    u, v = c * x + sn * y, -sn * x + c * y
    return u * u / (float(sigma_x) ** 2) + v * v / (float(sigma_y) ** 2)


def generalized_gaussian_kernel(size, sigma_x, sigma_y=None, theta=0.0, beta=1.0):
    """fp32 [size, size] generalised Gaussian ``exp(-0.5 q^beta)``, q = u^2 / sigma_x^2 + v^2 / sigma_y^2 in the rotated
    coordinates of ``gaussian_kernel`` (same grid, float64, normalised to sum 1, rounded to fp32 once).  ``beta == 1`` takes
    no power at all and equals ``gaussian_kernel`` bit for bit."""
    q = _rotated_q(size, sigma_x, sigma_y, theta, "generalized_gaussian_kernel")
    k = np.exp(-0.5 * (q if beta == 1 else np.power(q, float(beta))))
    return (k / k.sum()).astype(np.float32)


def plateau_kernel(size, sigma_x, sigma_y=None, theta=0.0, beta=1.0):
    """fp32 [size, size] plateau-shaped kernel ``1 / (q^beta + 1)`` with q as in ``generalized_gaussian_kernel``, normalised."""
    q = _rotated_q(size, sigma_x, sigma_y, theta, "plateau_kernel")
    k = 1.0 / (np.power(q, float(beta)) + 1.0)
    return (k / k.sum()).astype(np.float32)


_J1_TAU = (np.arange(128, dtype=np.float64) + 0.5) * (math.pi / 128)


def bessel_j1(x):
    """The Bessel function J1 in float64 by the midpoint rule on Bessel's integral, J1(x) = mean_k cos(tau_k - x sin tau_k),
    tau_k = (k + 1/2) pi / 128, k < 128: the integrand is smooth and periodic, so the rule converges geometrically (7.1e-16
    from scipy.special.j1 on [0, 45], the range ``sinc_kernel`` needs).  No scipy in the product."""
    x = np.asarray(x, dtype=np.float64)
    return np.cos(_J1_TAU - x[..., None] * np.sin(_J1_TAU)).mean(axis=-1)


def sinc_kernel64(cutoff, size):
    """``sinc_kernel`` before its rounding to fp32: float64 [size, size], normalised to sum 1"""
    size = int(size)
    if size < 1 or size % 2 == 0:
        raise ValueError(f"sinc_kernel: size {size} is not a positive odd number")
    cutoff = float(cutoff)
    if not cutoff > 0:
        raise ValueError("sinc_kernel: cutoff must be positive")
    r = size // 2
    y, x = np.meshgrid(np.arange(size, dtype=np.float64) - r, np.arange(size, dtype=np.float64) - r, indexing="ij")
    rho = np.hypot(x, y)
    rho[r, r] = 1.0
    k = cutoff * bessel_j1(cutoff * rho) / (2.0 * math.pi * rho)
    k[r, r] = cutoff * cutoff / (4.0 * math.pi)
    return k / k.sum()


def sinc_kernel(cutoff, size, pad_to=0):
    """fp32 circular low-pass (2-D sinc) filter ``cutoff J1(cutoff rho) / (2 pi rho)``, rho = hypot(x, y) on the grid of
    ``gaussian_kernel``, the centre tap ``cutoff^2 / (4 pi)``; float64, normalised to sum 1, rounded to fp32 once, then
    zero-padded symmetrically to [pad_to, pad_to] when pad_to > size."""
    return _pad_kernel(sinc_kernel64(cutoff, size).astype(np.float32), pad_to)


def _pad_kernel(k, pad_to):
    size = k.shape[0]
    if pad_to <= size:
        return k
    if (pad_to - size) % 2:
        raise ValueError(f"a {size}x{size} kernel cannot be padded symmetrically to {pad_to}")
    p = (pad_to - size) // 2
    return np.pad(k, ((p, p), (p, p)))


KERNEL_LIST = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")


def random_mixed_kernels(n, kernel_list=KERNEL_LIST, kernel_prob=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03), size=21, sigma_x=(0.2, 3.0),
                         sigma_y=(0.2, 3.0), rotation=(-math.pi, math.pi), betag=(0.5, 4.0), betap=(1.0, 2.0), sinc_prob=0.1,
                         rng=None, pad_to=21):
    """fp32 [n, pad_to, pad_to] kernels of the Real-ESRGAN family, made on the host.  Per sample, in this order, from `rng`
    (defaults to numpy's global generator; a seeded ``np.random.RandomState`` repeats itself):
      1. only when `size` is a sequence: ``rng.randint(len(size))`` picks the kernel size (the recipe: 7, 9, ..., 21);
      2. ``rng.uniform(0, 1)`` < sinc_prob takes the sinc branch: one more draw, the cutoff, uniform in [pi / 3, pi) for sizes
         below 13 and in [pi / 5, pi) otherwise -> ``sinc_kernel``; nothing else is drawn for this sample;
      3. otherwise ``rng.uniform(0, 1)`` picks the entry of `kernel_list` by the cumulative `kernel_prob` (normalised), then
         sigma_x, sigma_y and theta are drawn uniformly from their ranges, all three always (an ``*iso`` kernel uses sigma_x
         alone and no rotation);
      4. a ``generalized_*`` kernel draws ``rng.uniform(0, 1)`` < 0.5 and then beta uniform in [betag[0], 1) or, otherwise, in
         [1, betag[1]); a ``plateau_*`` kernel the same two draws with `betap`.
    Every kernel is normalised at its own size and then zero-padded symmetrically to `pad_to`."""
    rng = np.random if rng is None else rng
    names = tuple(kernel_list)
    for name in names:
        if name not in KERNEL_LIST:
            raise ValueError(f"random_mixed_kernels: unknown kernel {name!r}; one of {KERNEL_LIST}")
    prob = np.asarray(kernel_prob, dtype=np.float64)
    if prob.shape != (len(names),) or not (prob >= 0).all() or not prob.sum() > 0:
        raise ValueError("random_mixed_kernels: kernel_prob must hold one non-negative weight per kernel")
    cum = np.cumsum(prob / prob.sum())
    sizes = [int(s) for s in size] if isinstance(size, (tuple, list, np.ndarray)) else None
    for s in (sizes if sizes is not None else [int(size)]):
        if s < 1 or s % 2 == 0 or s > pad_to:
            raise ValueError(f"random_mixed_kernels: size {s} is not an odd number in 1..{pad_to}")

    def draw_beta(lo_hi):
        low = float(rng.uniform(0.0, 1.0)) < 0.5
        return float(rng.uniform(lo_hi[0], 1.0)) if low else float(rng.uniform(1.0, lo_hi[1]))

    out = np.zeros((n, pad_to, pad_to), dtype=np.float32)
    for b in range(n):
        ks = int(size) if sizes is None else sizes[int(rng.randint(len(sizes)))]
        if float(rng.uniform(0.0, 1.0)) < sinc_prob:
            cutoff = float(rng.uniform(math.pi / 3 if ks < 13 else math.pi / 5, math.pi))
            out[b] = sinc_kernel(cutoff, ks, pad_to)
            continue
        name = names[min(int(np.searchsorted(cum, float(rng.uniform(0.0, 1.0)), side="right")), len(names) - 1)]
        sx = float(rng.uniform(sigma_x[0], sigma_x[1]))
        sy = float(rng.uniform(sigma_y[0], sigma_y[1]))
        theta = float(rng.uniform(rotation[0], rotation[1]))
        if name.endswith("_iso") or name == "iso":
            sy, theta = sx, 0.0
        if name.startswith("generalized"):
            k = generalized_gaussian_kernel(ks, sx, sy, theta, draw_beta(betag))
        elif name.startswith("plateau"):
            k = plateau_kernel(ks, sx, sy, theta, draw_beta(betap))
        else:
            k = gaussian_kernel(ks, sx, sy, theta)
        out[b] = _pad_kernel(k, pad_to)
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


# ------------------------------------------------------------------ second-order Real-ESRGAN degradation (csrc/filter2d.hip,
# csrc/degrade_noise.hip): the stage functions that utils/realesrgan.py runs in sequence.  Data ops: no autograd.
def _batch_f32(x, who, channels=None):
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        raise TypeError(f"{who}: an fp32 [B, C, H, W] tensor is expected")
    if channels is not None and x.shape[1] != channels:
        raise TypeError(f"{who}: {channels} channels are expected, got {x.shape[1]}")
    _need_gpu(x)
    return x.detach().contiguous()


def filter2d(x, kernels):
    """BasicSR's ``filter2D``: fp32 [B, C, H, W] device batch correlated with a kernel per sample (fp32 [B, ks, ks]) or with one
    kernel for all ([ks, ks]), borders reflected as torch's 'reflect'; a new tensor.  ks odd in 1..21 and H, W >= ks // 2 + 1.
    One fmaf per tap in row-major tap order (dsr_filter2d_f32): the result is defined bit for bit, and a kernel zero-padded
    to a larger size gives the bits of the kernel itself.  Kernels may be numpy arrays (uploaded once)."""
    x = _batch_f32(x, "filter2d")
    k = torch.from_numpy(np.ascontiguousarray(kernels, dtype=np.float32)) if isinstance(kernels, np.ndarray) else kernels
    if not torch.is_tensor(k) or k.dtype != torch.float32 or k.dim() not in (2, 3) or k.shape[-1] != k.shape[-2]:
        raise ValueError("filter2d: kernels must be fp32 [B, ks, ks] or [ks, ks]")
    b, c, h, w = (int(v) for v in x.shape)
    shared = k.dim() == 2
    if not shared and k.shape[0] != b:
        raise ValueError(f"filter2d: {k.shape[0]} kernels for {b} samples")
    ks = int(k.shape[-1])
    if ks % 2 == 0 or ks > KERNEL_SIZE_MAX:
        raise ValueError(f"filter2d: kernel size {ks} is not an odd number in 1..{KERNEL_SIZE_MAX}")
    if min(h, w) < ks // 2 + 1:
        raise ValueError(f"filter2d: a {ks}x{ks} kernel cannot be reflected in a {h}x{w} image")
    k = k.to(x.device).contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().dsr_filter2d_f32(_ptr(x), _ptr(y), _ptr(k), b, c, h, w, ks, int(shared), _stream()))
    return y


def _per_sample(v, n, device, dtype, who):
    """-> contiguous `dtype` [n] on `device` from a scalar, a sequence or a tensor"""
    if not torch.is_tensor(v):
        v = torch.tensor([v] * n if isinstance(v, (int, float, bool, np.integer, np.floating, np.bool_)) else list(v))
    if v.numel() != n:
        raise ValueError(f"{who}: {v.numel()} values for {n} samples")
    return v.reshape(n).to(device=device, dtype=dtype).contiguous()


def _draw_like(shape, given, x, who):
    if given is None:
        return None
    if not (torch.is_tensor(given) and given.dtype == torch.float32 and tuple(given.shape) == tuple(shape)):
        raise ValueError(f"{who}: a draw must be fp32 {tuple(shape)}")
    return given.to(x.device).contiguous()


def add_gaussian_noise_batch(x, sigma, gray, generator=None, z=None, zg=None):
    """Real-ESRGAN's Gaussian noise on an fp32 [B, 3, H, W] device batch in [0, 1] scaling (dsr_noise_gaussian_f32; a new
    tensor): ``clamp(x + sigma_b / 255 * n, 0, 1)`` with n = z, fp32 [B, 3, H, W], or, for a sample whose `gray` flag is set,
    zg, fp32 [B, H, W], on all three channels.  sigma (0..255 units) and gray: per sample, scalars, sequences or device
    tensors (not read back).  The draws z and then zg are ``torch.randn`` on the device from `generator`; given ones are used
    as they are."""
    x = _batch_f32(x, "add_gaussian_noise_batch", 3)
    b, _, h, w = (int(v) for v in x.shape)
    sigma = _per_sample(sigma, b, x.device, torch.float32, "add_gaussian_noise_batch: sigma")
    gray = _per_sample(gray, b, x.device, torch.uint8, "add_gaussian_noise_batch: gray")
    z = _draw_like((b, 3, h, w), z, x, "add_gaussian_noise_batch")
    zg = _draw_like((b, h, w), zg, x, "add_gaussian_noise_batch")
    if z is None:
        z = torch.randn((b, 3, h, w), dtype=torch.float32, device=x.device, generator=generator)
    if zg is None:
        zg = torch.randn((b, h, w), dtype=torch.float32, device=x.device, generator=generator)
    y = torch.empty_like(x)
    check(_lib.lib().dsr_noise_gaussian_f32(_ptr(x), _ptr(z), _ptr(zg), _ptr(sigma), _ptr(gray), _ptr(y), b, h, w, _stream()))
    return y


_GRAY_WEIGHTS = (0.2989, 0.587, 0.114)


def poisson_levels(x, gray):
    """(q, g, vals) of ``add_poisson_noise_batch`` from torch ops on x's device, with no host read: q = round(clamp(255 x, 0,
    255)) / 255, fp32 [B, 3, H, W]; g = 0.2989 q_r + 0.587 q_g + 0.114 q_b, fp32 [B, H, W]; vals, fp32 [B], the smallest power
    of two that is >= the number of distinct grey levels of the sample -- of round(255 q) over its three channels, or, for a
    sample whose `gray` flag is set, of round(255 g): ``2 ** ceil(log2(len(unique(plane))))``."""
    q = torch.round(torch.clamp(x * 255.0, 0.0, 255.0)) / 255.0
    g = _GRAY_WEIGHTS[0] * q[:, 0] + _GRAY_WEIGHTS[1] * q[:, 1] + _GRAY_WEIGHTS[2] * q[:, 2]
    b = x.shape[0]

    def distinct(levels):                                            # int64 [B, n] in 0..255 -> how many differ, per row
        seen = torch.zeros((b, 256), dtype=torch.float32, device=x.device)
        seen.scatter_(1, levels, 1.0)
        return seen.sum(dim=1)

    count_c = distinct(torch.round(q * 255.0).to(torch.int64).reshape(b, -1))
    count_g = distinct(torch.round(g * 255.0).clamp_(0.0, 255.0).to(torch.int64).reshape(b, -1))
    count = torch.where(gray.to(torch.bool), count_g, count_c)
    powers = torch.tensor([float(1 << e) for e in range(9)], dtype=torch.float32, device=x.device)      # 1 .. 256
    vals = torch.exp2((count[:, None] > powers[None, :]).sum(dim=1).to(torch.float32))
    return q, g, vals


def add_poisson_noise_batch(x, scale, gray, generator=None, z=None, zg=None, vals=None):
    """Real-ESRGAN's Poisson (shot) noise on an fp32 [B, 3, H, W] device batch in [0, 1] scaling (dsr_noise_poisson_f32; a
    new tensor).  With q, g and vals of ``poisson_levels``: colour samples add ``scale_b * (z / vals_b - q)``, z ~
    Poisson(q vals_b); samples whose `gray` flag is set add ``scale_b * (zg / vals_b - g)`` to all three channels, zg ~
    Poisson(g vals_b); then clamp to [0, 1].  The draws (z, then zg: ``torch.poisson`` on the device from `generator`) and
    vals are made here unless given, without a host read."""
    x = _batch_f32(x, "add_poisson_noise_batch", 3)
    b, _, h, w = (int(v) for v in x.shape)
    scale = _per_sample(scale, b, x.device, torch.float32, "add_poisson_noise_batch: scale")
    gray = _per_sample(gray, b, x.device, torch.uint8, "add_poisson_noise_batch: gray")
    z = _draw_like((b, 3, h, w), z, x, "add_poisson_noise_batch")
    zg = _draw_like((b, h, w), zg, x, "add_poisson_noise_batch")
    if vals is not None:
        vals = _per_sample(vals, b, x.device, torch.float32, "add_poisson_noise_batch: vals")
    if z is None or zg is None or vals is None:
        q, g, own = poisson_levels(x, gray)
        vals = own if vals is None else vals
        if z is None:
            z = torch.poisson(q * vals[:, None, None, None], generator=generator)
        if zg is None:
            zg = torch.poisson(g * vals[:, None, None], generator=generator)
    y = torch.empty_like(x)
    check(_lib.lib().dsr_noise_poisson_f32(_ptr(x), _ptr(z), _ptr(zg), _ptr(vals), _ptr(scale), _ptr(gray), _ptr(y), b, h, w,
                                           _stream()))
    return y


# ------------------------------------------------------------------ unsharp mask
_usm_cache = {}


def usm_kernel(radius=50, sigma=0):
    """OpenCV's ``getGaussianKernel(radius, sigma)`` as float64 [k]: an even radius is made odd (k = radius + 1), sigma <= 0
    means 0.3 ((k - 1) / 2 - 1) + 0.8; ``exp(-(i - (k - 1) / 2)^2 / (2 sigma^2))`` normalised to sum 1."""
    k = int(radius)
    if k < 1:
        raise ValueError(f"usm_kernel: radius {radius}")
    if k % 2 == 0:
        k += 1
    s = float(sigma) if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * s * s))
    return g / g.sum()


def _usm_tables(n, radius, sigma, device):
    """``AxisTables`` of the 1-D blur at unchanged size n: k taps per output with torch-'reflect'ed indices (cached)."""
    from .imresize import AxisTables
    key = (int(n), int(radius), float(sigma), str(device))
    hit = _usm_cache.get(key)
    if hit is None:
        g = usm_kernel(radius, sigma)
        r = g.shape[0] // 2
        pos = np.arange(n, dtype=np.int64)[:, None] + np.arange(-r, r + 1, dtype=np.int64)[None, :]
        pos = np.abs(pos)
        pos = np.where(pos > n - 1, 2 * (n - 1) - pos, pos)
        hit = _usm_cache[key] = AxisTables(n, n, 1.0, np.ascontiguousarray(np.broadcast_to(g, pos.shape)), pos, device)
    return hit


def usm_sharp(x, weight=0.5, threshold=10, radius=50, sigma=0):
    """BasicSR's ``USMSharp`` on an fp32 [B, C, H, W] device batch in [0, 1] scaling; a new tensor.  With G the Gaussian of
    ``usm_kernel`` (51 taps, sigma 8 at the defaults), borders reflected:
        blur = G * x;  res = x - blur;  mask = |res| 255 > threshold;  soft = G * mask
        sharp = clamp(x + weight res, 0, 1);  y = soft sharp + (1 - soft) x
    G is rank 1, and the blur is defined here as the separable pass, rows of taps along H and then along W: the separable
    form of BasicSR's 51 x 51 ``filter2D``, equal to it up to rounding.  Four launches: dsr_imresize_f32 at unchanged size
    with k-tap tables for each blur, dsr_usm_mask, dsr_usm_combine; no res or sharp tensor exists.  H, W >= k // 2 + 1 (26 at
    the defaults), otherwise ValueError; k <= 63."""
    from ..functional import _imresize_launch
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        raise TypeError("usm_sharp: an fp32 [B, C, H, W] tensor is expected")
    k = usm_kernel(radius, sigma).shape[0]
    b, c, h, w = (int(v) for v in x.shape)
    if min(h, w) < k // 2 + 1:
        raise ValueError(f"usm_sharp: a {k}-tap blur cannot be reflected in a {h}x{w} image ({k // 2 + 1} pixels are needed)")
    _need_gpu(x)
    x = x.detach().contiguous()
    th, tw = _usm_tables(h, radius, sigma, x.device), _usm_tables(w, radius, sigma, x.device)
    lib = _lib.lib()
    blur, mask, soft, y = (torch.empty_like(x) for _ in range(4))
    _imresize_launch(x, blur, b * c, h, w, h, w, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)
    check(lib.dsr_usm_mask(_ptr(x), _ptr(blur), float(threshold), _ptr(mask), x.numel(), _stream()))
    _imresize_launch(mask, soft, b * c, h, w, h, w, th.idx, th.w, th.taps, tw.idx, tw.w, tw.taps)
    check(lib.dsr_usm_combine(_ptr(x), _ptr(blur), _ptr(soft), float(weight), _ptr(y), x.numel(), _stream()))
    return y


class USMSharp(torch.nn.Module):
    """``usm_sharp`` as a module with the same arguments: no parameters, no buffers."""

    def __init__(self, weight=0.5, threshold=10, radius=50, sigma=0):
        super().__init__()
        usm_kernel(radius, sigma)
        self.weight, self.threshold, self.radius, self.sigma = float(weight), float(threshold), int(radius), float(sigma)

    def forward(self, x):
        return usm_sharp(x, self.weight, self.threshold, self.radius, self.sigma)

    def extra_repr(self):
        return f"weight={self.weight}, threshold={self.threshold}, radius={self.radius}, sigma={self.sigma}"
