"""Float64 restatement of multi-scale SSIM per image (test infrastructure, differentiable), built on tests/ssim_ref.py's window
and moments: torchmetrics' MultiScaleStructuralSimilarityIndexMeasure as the package's docstrings state it (torchmetrics is
absent, so this pins the package's own definition, not torchmetrics' bits).

Per scale s = 0 .. L-1 on the current pair: cs_map = (2 cov + c2) / (var_a + var_b + c2) and ssim_map = cs_map * (2 mu_a mu_b +
c1) / (mu_a^2 + mu_b^2 + c1) at every window position inside the image, their per-image means, clamped at 0 under 'relu'; then
both images become F.avg_pool2d(x, 2).  v = (cs_0 .. cs_{L-2}, ssim_{L-1}), (v + 1) / 2 under 'simple'; the value is
prod_s v_s ** betas[s].  Written with F.conv2d / F.avg_pool2d, so torch autograd of it is the reference gradient; it runs in
whatever dtype its inputs have (float64 for the reference, float32 for the storage-model floor)."""
import torch
import torch.nn.functional as F

import ssim_ref

DEFAULT_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def ssim_cs_maps(a, b, data_range=1.0, k1=0.01, k2=0.03):
    """([N,C,H-10,W-10] ssim_map, cs_map): the moments and constants of ssim_ref.ssim_map, as the two factors."""
    c = a.shape[1]
    g = ssim_ref.gaussian_window(dtype=a.dtype).to(a.device)
    win = (g[:, None] * g[None, :])[None, None].expand(c, 1, 11, 11)
    mu_a, mu_b = F.conv2d(a, win, groups=c), F.conv2d(b, win, groups=c)
    s_aa = F.conv2d(a * a, win, groups=c) - mu_a * mu_a
    s_bb = F.conv2d(b * b, win, groups=c) - mu_b * mu_b
    s_ab = F.conv2d(a * b, win, groups=c) - mu_a * mu_b
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    cs = (2 * s_ab + c2) / (s_aa + s_bb + c2)
    return cs * ((2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)), cs


def raw_scales(a, b, levels, data_range=1.0, k1=0.01, k2=0.03):
    """[L, N]: the per-image cs means of scales 0 .. L-2 and the per-image SSIM mean of scale L-1, before any normalisation."""
    rows = []
    for s in range(levels):
        sim, cs = ssim_cs_maps(a, b, data_range, k1, k2)
        rows.append((sim if s == levels - 1 else cs).mean(dim=(1, 2, 3)))
        if s < levels - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return torch.stack(rows)


def msssim_per_image(a, b, betas=DEFAULT_BETAS, normalize="relu", data_range=1.0, k1=0.01, k2=0.03):
    """([N] value of each image pair, [L, N] the normalised per-scale values that enter the powers)."""
    v = raw_scales(a, b, len(betas), data_range, k1, k2)
    if normalize == "relu":
        v = torch.relu(v)
    elif normalize == "simple":
        v = (v + 1) / 2
    else:
        assert normalize is None, normalize
    bt = torch.tensor(betas, dtype=v.dtype, device=v.device).view(-1, 1)
    return torch.prod(v ** bt, dim=0), v


def textured_pair(shape, noise, seed):
    """(preds, target) in float64: a smooth image plus a texture of amplitude 0.3 as the target, the target plus uniform noise as
    the prediction.  `noise`: the amplitude (peak to peak), one number or one per image.  For amplitudes in [0.05, 1] every
    per-scale value of the default five scales stays above 0.15 (the lowest, cs of scale 0 at amplitude 1, is 0.156), so no
    case sits on the 'relu' clamp or on the steep end of v ** 0.0448."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    yy = torch.linspace(0, 1, h, dtype=torch.float64).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, dtype=torch.float64).view(1, 1, 1, w)
    ph = torch.rand(n, c, 1, 1, generator=g, dtype=torch.float64)
    t = 0.5 + 0.3 * torch.sin(6.0 * (yy + ph)) * torch.cos(5.0 * (xx - ph))
    t = t + 0.3 * (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5)
    amp = torch.as_tensor(noise, dtype=torch.float64).reshape(-1, 1, 1, 1)
    p = t + amp * (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5)
    return p, t
