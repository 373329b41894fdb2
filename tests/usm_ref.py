"""Float64 yardstick of utils.degradation.usm_sharp from torch CPU ops: OpenCV's getGaussianKernel written out, the blur as
F.pad(mode='reflect') + F.conv2d along H and then along W.  Nothing here comes from the product."""
import torch
import torch.nn.functional as F


def gaussian_1d(radius=50, sigma=0):
    k = radius + 1 if radius % 2 == 0 else radius
    s = sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = torch.arange(k, dtype=torch.float64) - (k - 1) / 2
    g = torch.exp(-(i * i) / (2 * s * s))
    return g / g.sum()


def blur(x, g):
    b, c, h, w = x.shape
    r = g.numel() // 2
    x = x.reshape(b * c, 1, h, w)
    x = F.conv2d(F.pad(x, (0, 0, r, r), mode="reflect"), g.reshape(1, 1, -1, 1))
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="reflect"), g.reshape(1, 1, 1, -1))
    return x.reshape(b, c, h, w)


def usm_sharp(x, weight=0.5, threshold=10, radius=50, sigma=0):
    """-> (y, mask, margin): float64 result, the boolean mask and min | |res| 255 - threshold | over all pixels"""
    x = torch.as_tensor(x).double()
    g = gaussian_1d(radius, sigma)
    res = x - blur(x, g)
    level = res.abs() * 255.0
    mask = level > threshold
    soft = blur(mask.double(), g)
    sharp = torch.clamp(x + weight * res, 0.0, 1.0)
    return soft * sharp + (1.0 - soft) * x, mask, float((level - threshold).abs().min())
