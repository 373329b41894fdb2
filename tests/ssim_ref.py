"""Float64 restatement of SSIM per image (test infrastructure, differentiable): the definition of oracle/metrics.py
(Gaussian 11x11 window, sigma 1.5, K1 = 0.01, K2 = 0.03, per channel, window positions inside the image) with the mean taken
over each image's C x (H-10) x (W-10) positions instead of the whole batch.  Written with F.conv2d, so torch autograd of it is
the reference gradient of the GPU tests; it runs in whatever dtype its inputs have (float64 for the reference, float32 for the
storage-model floor)."""
import torch
import torch.nn.functional as F


def gaussian_window(size=11, sigma=1.5, dtype=torch.float64):
    d = torch.arange(size, dtype=torch.float64) - (size - 1) / 2.0
    g = torch.exp(-d * d / (2.0 * sigma * sigma))
    return (g / g.sum()).to(dtype)


def ssim_map(a, b, data_range=1.0, k1=0.01, k2=0.03):
    """[N,C,H-10,W-10] SSIM at every window position inside the image (unclamped formula)."""
    c = a.shape[1]
    g = gaussian_window(dtype=a.dtype).to(a.device)
    win = (g[:, None] * g[None, :])[None, None].expand(c, 1, 11, 11)
    mu_a, mu_b = F.conv2d(a, win, groups=c), F.conv2d(b, win, groups=c)
    s_aa = F.conv2d(a * a, win, groups=c) - mu_a * mu_a
    s_bb = F.conv2d(b * b, win, groups=c) - mu_b * mu_b
    s_ab = F.conv2d(a * b, win, groups=c) - mu_a * mu_b
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    return ((2 * mu_a * mu_b + c1) * (2 * s_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))


def ssim_per_image(a, b, data_range=1.0, k1=0.01, k2=0.03):
    """[N]: mean SSIM of each image pair."""
    return ssim_map(a, b, data_range, k1, k2).mean(dim=(1, 2, 3))
