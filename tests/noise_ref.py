"""Float64 yardstick of the noise application of the second-order degradation (utils.degradation.add_gaussian_noise_batch /
add_poisson_noise_batch) from torch CPU ops; the draws are inputs.  Nothing here comes from the product."""
import torch


def _per(v, like):
    return torch.as_tensor(v).double().reshape(-1, *([1] * (like.dim() - 1)))


def gaussian(x, z, zg, sigma, gray):
    """-> (y, noise term) float64: y = clamp(x + sigma / 255 * (gray ? zg : z), 0, 1)"""
    x, z, zg = (torch.as_tensor(t).double() for t in (x, z, zg))
    g = torch.as_tensor(gray).bool().reshape(-1, 1, 1, 1)
    term = _per(sigma, x) / 255.0 * torch.where(g, zg[:, None].expand_as(z), z)
    return torch.clamp(x + term, 0.0, 1.0), term


def quantised(x):
    return torch.round(torch.clamp(torch.as_tensor(x).double() * 255.0, 0.0, 255.0)) / 255.0


def grey(q):
    return 0.2989 * q[:, 0] + 0.587 * q[:, 1] + 0.114 * q[:, 2]


def poisson(x, z, zg, vals, scale, gray):
    """-> (y, noise term) float64.  q = round(clamp(255 x)) / 255; colour n = z / vals - q; grey n = zg / vals - grey(q)"""
    x, z, zg = (torch.as_tensor(t).double() for t in (x, z, zg))
    q = quantised(x)
    g = torch.as_tensor(gray).bool().reshape(-1, 1, 1, 1)
    v = _per(vals, x)
    n = torch.where(g, (zg / v[:, 0] - grey(q))[:, None].expand_as(z), z / v - q)
    term = _per(scale, x) * n
    return torch.clamp(x + term, 0.0, 1.0), term


def vals(x, gray_flag):
    """2 ** ceil(log2(number of distinct grey levels)) of ONE sample x [3, H, W]: of its quantised channels, or of its quantised
    grey plane round(255 grey(q)) when gray_flag"""
    q = quantised(x)
    plane = torch.round(grey(q[None])[0] * 255.0) if gray_flag else torch.round(q * 255.0)
    return 2.0 ** int(torch.ceil(torch.log2(torch.tensor(float(len(torch.unique(plane)))))).item())
