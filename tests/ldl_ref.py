"""Float64 CPU yardstick of the LDL artifact-map loss (functional.ldl_loss / ldl_artifact_map, csrc/ldl.hip) and of
steps.realesrgan_step's generator loss with that term.

"Details or Artifacts: A Locally Discriminative Learning Approach" (CVPR 2022) as BasicSR's ldl_opt states it, restated: parity
with BasicSR is unpinned.  Two statements of the same thing:

  literal_*   pad / unfold / var / index-assign / l1_loss, differentiated by torch autograd
  closed_*    the sums the kernel evaluates (include/dsr_hip.h), with the gradient written out

tests/test_host_ldl.py holds the closed form to autograd of the literal one.  Both run in the dtype of their operands (float64:
the yardstick; float32: the floor of the GPU tests).  Nothing is imported from the package under test."""
import contextlib

import torch
import torch.nn.functional as TF


# ----------------------------------------------------------------------------- the literal form
def residuals(x, gt, e):
    """r = sum_c |gt - x| and re = sum_c |gt - e|, [N, 1, H, W]; the channels are added in channel order."""
    dx, de = (gt - x).abs(), (gt - e).abs()
    r, re = dx[:, :1].clone(), de[:, :1].clone()
    for c in range(1, x.shape[1]):
        r = r + dx[:, c:c + 1]
        re = re + de[:, c:c + 1]
    return r, re


def local_variance(r, k):
    """Unbiased variance of r [N, 1, H, W] over the k x k window of the reflect-padded plane."""
    p = (k - 1) // 2
    win = TF.pad(r, [p, p, p, p], mode="reflect").unfold(2, k, 1).unfold(3, k, 1)
    return win.var(dim=(-1, -2), unbiased=True)


def literal_map(x, gt, e, k=7):
    """The refined artifact map w [N, 1, H, W]: var(r[n])^(1/5) * local variance, zero where r < re."""
    r, re = residuals(x, gt, e)
    patch = r.var(dim=(-1, -2, -3), keepdim=True, unbiased=True) ** (1 / 5)
    w = patch * local_variance(r, k)
    w[r < re] = 0
    return w


def literal_loss(x, gt, e, k=7, detach_weight=False):
    w = literal_map(x, gt, e, k)
    if detach_weight:
        w = w.detach()
    return TF.l1_loss(w * x, w * gt)


# ----------------------------------------------------------------------------- the closed form
def box_sum(a, k):
    """Sum over the k x k window of the reflect-padded plane a [N, 1, H, W]."""
    p = (k - 1) // 2
    return TF.avg_pool2d(TF.pad(a, [p, p, p, p], mode="reflect"), k, stride=1, divisor_override=1)


def box_sum_adjoint(c, k):
    """The adjoint of box_sum: a box sum of the zero-extended plane on the padded domain, then the p reflected border rows and
    columns folded back onto rows / columns 1..p and H-2..H-1-p."""
    p = (k - 1) // 2
    H, W = c.shape[-2:]
    d = TF.avg_pool2d(TF.pad(c, [2 * p] * 4), k, stride=1, divisor_override=1)          # [.., H + 2p, W + 2p]: the padded domain
    out = d[..., p:p + H, :].clone()
    for j in range(1, p + 1):
        out[..., j, :] += d[..., p - j, :]
        out[..., H - 1 - j, :] += d[..., p + H - 1 + j, :]
    d = out
    out = d[..., :, p:p + W].clone()
    for j in range(1, p + 1):
        out[..., :, j] += d[..., :, p - j]
        out[..., :, W - 1 - j] += d[..., :, p + W - 1 + j]
    return out


def closed_parts(x, gt, e, k=7):
    """r, mask m, window mean mu, window variance v (two-pass), and per image rbar, V, g = V^(1/5), S = sum m r v."""
    K = k * k
    r, re = residuals(x, gt, e)
    m = (~(r < re)).to(r.dtype)
    mu = box_sum(r, k) / K
    p = (k - 1) // 2
    win = TF.pad(r, [p, p, p, p], mode="reflect").unfold(2, k, 1).unfold(3, k, 1)
    v = ((win - mu[..., None, None]) ** 2).sum(dim=(-1, -2)) / (K - 1)
    rbar = r.mean(dim=(1, 2, 3), keepdim=True)
    hw = r.shape[-1] * r.shape[-2]
    V = ((r - rbar) ** 2).sum(dim=(1, 2, 3), keepdim=True) / (hw - 1)
    g = V ** (1 / 5)
    S = (m * r * v).sum(dim=(1, 2, 3), keepdim=True)
    return r, m, mu, v, rbar, V, g, S


def closed_map(x, gt, e, k=7):
    r, m, mu, v, rbar, V, g, S = closed_parts(x, gt, e, k)
    return torch.where(V == 0, torch.zeros_like(v), g * v * m)


def closed_loss_and_grad(x, gt, e, k=7, detach_weight=False):
    """(loss, dloss/dx) of the closed form; an image whose r is constant (V == 0) adds 0 to both."""
    K, M = k * k, x.numel()
    r, m, mu, v, rbar, V, g, S = closed_parts(x, gt, e, k)
    flat = V == 0
    zero = torch.zeros_like(V)
    loss = torch.where(flat, zero, g * S).sum() / M
    w = g * v * m
    if detach_weight:
        dr = w
    else:
        hw = r.shape[-1] * r.shape[-2]
        t2 = (2.0 / (K - 1)) * g * (r * box_sum_adjoint(m * r, k) - box_sum_adjoint(m * r * mu, k))
        safe = torch.where(flat, torch.ones_like(V), V)
        t3 = S * (1 / 5) * safe ** (-4 / 5) * 2 * (r - rbar) / (hw - 1)
        dr = w + t2 + t3
    dr = torch.where(flat, torch.zeros_like(dr), dr) / M
    return loss, torch.sign(x - gt) * dr


# ----------------------------------------------------------------------------- test inputs
def grid_inputs(shape, seed):
    """x, gt, e on the grid of multiples of 1/256 in [0, 1]: r, re and the mask are exact in fp32.  Planted: ties r == re (e = x
    on every 7th pixel), elements x == gt (every 5th), whose gradient is 0."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 257, shape, generator=g).float() / 256
    x = torch.randint(0, 257, shape, generator=g).float() / 256
    e = torch.randint(0, 257, shape, generator=g).float() / 256
    flat_x, flat_e, flat_gt = x.view(shape[0], shape[1], -1), e.view(shape[0], shape[1], -1), gt.view(shape[0], shape[1], -1)
    flat_e[:, :, ::7] = flat_x[:, :, ::7]
    flat_x.view(-1)[::5] = flat_gt.reshape(-1)[::5]
    return x, gt, e


def noise_inputs(shape, seed):
    """gt uniform in [0, 1], x and e = gt + 0.1 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    x = gt + 0.1 * torch.randn(shape, generator=g)
    e = gt + 0.1 * torch.randn(shape, generator=g)
    return x, gt, e


# ----------------------------------------------------------------------------- the step
def step_reference(gsd, esd, dsd, vsd, lq, gt, dtype, layer_weights, l1_weight, gan_weight, ldl_weight, k=7, detach_weight=False):
    """steps.realesrgan_step(ldl_weight=..., gen_ema=...) in float64 (dtype=None) or under the bf16 storage model, restated on
    the yardsticks of tests/test_gpu_unetd.py: the six losses (l_pix, l_percep, l_g_gan, l_d_real, l_d_fake, l_g_ldl), the
    generator's gradients and the generator's output.  esd: the state of the EMA generator as it stands BEFORE the step."""
    import rrdb_ref as R
    import unetd_ref as U
    import vggfeat_ref
    from oracle import lowp

    leaves = {k_: v.double().clone().requires_grad_(True) for k_, v in gsd.items()}
    gt64 = gt.double()
    with torch.no_grad():
        fake_ema = R.network({k_: v.double() for k_, v in esd.items()}, lq, 4, dtype=dtype, fused=False)
    fake = R.network(leaves, lq, 4, dtype=dtype, fused=False)
    l_pix = (fake - gt64).abs().mean()
    ctx = lowp.storage(torch.bfloat16) if dtype is not None else contextlib.nullcontext()
    with ctx:
        l_percep = vggfeat_ref.ref_loss({k_: v.double() for k_, v in vsd.items()}, fake, gt64, layer_weights, "l1", True, False)
    d = {k_: v.double().clone() for k_, v in dsd.items()}

    def disc(img):
        y, vec = U.network(d, img, dtype, True, True)
        for name, (u, v) in vec.items():
            d[name + ".weight_u"], d[name + ".weight_v"] = u, v
        return y

    l_g_gan = U.gan_loss(disc(fake), True)
    l_g_ldl = literal_loss(fake, gt64, fake_ema, k, detach_weight)
    (l1_weight * l_pix + l_percep + gan_weight * l_g_gan + ldl_weight * l_g_ldl).backward()
    grads = {k_: v.grad for k_, v in leaves.items()}
    with torch.no_grad():
        l_d_real = U.gan_loss(disc(gt64), True, "vanilla", True)
        l_d_fake = U.gan_loss(disc(fake.detach()), False, "vanilla", True)
    losses = [float(v.detach()) for v in (l_pix, l_percep, l_g_gan, l_d_real, l_d_fake, l_g_ldl)]
    return losses, grads, fake.detach()
