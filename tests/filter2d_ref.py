"""Float64 yardstick of utils.degradation.filter2d from torch CPU ops: F.pad(mode='reflect') + a grouped F.conv2d (a
correlation, as torch's convolution is).  Nothing here comes from the product."""
import torch
import torch.nn.functional as F


def filter2d(x, kernels):
    """x: [B, C, H, W]; kernels: [B, ks, ks], or [ks, ks] for every sample -> float64 [B, C, H, W]"""
    x = torch.as_tensor(x).double()
    k = torch.as_tensor(kernels).double()
    b, c, h, w = x.shape
    if k.dim() == 2:
        k = k[None].expand(b, -1, -1)
    ks = k.shape[-1]
    r = ks // 2
    xp = F.pad(x, (r, r, r, r), mode="reflect") if r else x
    weight = k[:, None].expand(b, c, ks, ks).reshape(b * c, 1, ks, ks)
    y = F.conv2d(xp.reshape(1, b * c, h + 2 * r, w + 2 * r), weight, groups=b * c)
    return y.reshape(b, c, h, w)


def bound(kernels, x):
    """(ks^2 + 2) 2^-24 sum|k| max|x|: one rounding per fmaf, each on a partial sum no larger than sum|k| max|x|, plus the
    rounding of the float64 reference to fp32 and slack for second-order terms."""
    k = torch.as_tensor(kernels).double()
    ks = k.shape[-1]
    return (ks * ks + 2) * 2.0 ** -24 * float(k.abs().reshape(-1, ks * ks).sum(dim=1).max()) * float(torch.as_tensor(x).abs().max())
