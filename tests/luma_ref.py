"""The yardstick of the Y-channel metrics (test infrastructure): the evaluation protocol of the published super-resolution
tables restated on the CPU.  The 8-bit quantisation is done in fp32 torch, ``(x.float().clamp(0, 1) * 255).round()`` -- one fp32
multiply, round half to even, the integer ``evaluate.to_uint8_image`` writes; everything after it is float64: the division by
255, the BT.601 luma ``(16 + 65.481 r + 128.553 g + 24.966 b) / 255`` of MATLAB's ``rgb2ycbcr``, the border crop, the per-image
MSE and PSNR, and SSIM with the 11x11 sigma-1.5 Gaussian on the valid positions (tests/ssim_ref.py)."""
import math

import torch

import ssim_ref

WEIGHTS = (65.481, 128.553, 24.966)
OFFSET = 16.0


def quantise(x, quantize):
    """float64 [N,3,H,W]: q(x) = round(clamp(x, 0, 1) * 255) / 255 with the rounding done in fp32, or x itself."""
    if not quantize:
        return x.double()
    return (x.float().clamp(0.0, 1.0) * 255.0).round().double() / 255.0


def crop(x, shave):
    return x[..., shave:x.shape[-2] - shave, shave:x.shape[-1] - shave]


def rgb_to_y(x, shave=0, quantize=False):
    """float64 [N,1,H-2s,W-2s]."""
    q = crop(quantise(x, quantize), shave)
    y = (OFFSET + WEIGHTS[0] * q[:, 0] + WEIGHTS[1] * q[:, 1] + WEIGHTS[2] * q[:, 2]) / 255.0
    return y[:, None]


def psnr_y(preds, target, shave=0, quantize=True):
    """float64 [N]: 10 log10(1 / mean((Y(p) - Y(t))^2)) per image over the cropped region; +inf for identical images."""
    d = rgb_to_y(preds, shave, quantize) - rgb_to_y(target, shave, quantize)
    mse = (d * d).mean(dim=(1, 2, 3))
    return torch.tensor([10.0 * math.log10(1.0 / m) if m > 0 else math.inf for m in mse.tolist()], dtype=torch.float64)


def ssim_y(preds, target, shave=0, quantize=True):
    """float64 [N]: per-image SSIM (data_range 1) of the two cropped luma planes."""
    return ssim_ref.ssim_per_image(rgb_to_y(preds, shave, quantize), rgb_to_y(target, shave, quantize), 1.0)
