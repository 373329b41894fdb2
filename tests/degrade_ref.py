"""Yardstick of the blind-degradation kernel (csrc/degrade.hip): torch on the CPU in float64.

  blur(img, k, s, offset)       F.pad(mode='reflect') -> F.conv2d with the fp32 kernel values widened to float64 -> [offset::s]
  finish(acc, z, std, quantise) + std * z -> clip to 0..255 -> round half to even              (0..255 units, float64)
  scale_f32(v255, mode)         the scaling statements of patch_batch_kernel in float32, statement for statement (numpy float32
                                arithmetic rounds every statement once, as the kernel does): for the exact tests
F.conv2d is a cross-correlation: out[y][x] = sum k[i][j] * padded[y + i][x + j], the definition in include/dsr_hip.h."""
import numpy as np
import torch
import torch.nn.functional as F

UNIT, LR_REF, HR_REF, HR_UNIT = range(4)


def blur(img, kernel, s, offset=0):
    """img uint8 [H, W, 3] (tensor or array), kernel fp32 [ks, ks] -> float64 [3, h, w], h = ceil((H - offset) / s)"""
    x = torch.as_tensor(np.asarray(img)).permute(2, 0, 1).to(torch.float64)[None]
    k = torch.as_tensor(np.asarray(kernel))
    assert k.dtype == torch.float32 and k.dim() == 2 and k.shape[0] == k.shape[1] and k.shape[0] % 2 == 1
    r = k.shape[0] // 2
    x = F.pad(x, (r, r, r, r), mode="reflect") if r else x
    w = k.to(torch.float64)[None, None].expand(3, 1, -1, -1).contiguous()
    return F.conv2d(x, w, groups=3)[0][:, offset::s, offset::s].contiguous()


def finish(acc, z=None, std=0.0, quantise=True):
    """acc float64 [3, h, w] -> after noise (std: an fp32 value, z: fp32 [3, h, w]), clip and (optionally) rounding"""
    if z is not None:
        acc = acc + float(np.float32(std)) * torch.as_tensor(np.asarray(z)).to(torch.float64)
    acc = acc.clamp(0.0, 255.0)
    return torch.round(acc) if quantise else acc


def degrade(img, kernel, s, offset=0, z=None, std=0.0, quantise=True):
    return finish(blur(img, kernel, s, offset), z, std, quantise)


def scale_f32(v255, mode):
    """float64 values that ARE fp32 numbers (checked) -> what the kernel stores: v = acc / 255.0f, then the mode statements"""
    a = np.asarray(v255, dtype=np.float64)
    v = a.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), a), "scale_f32 is for values that fp32 holds exactly"
    f255, two, one = np.float32(255.0), np.float32(2.0), np.float32(1.0)
    v = v / f255
    if mode == LR_REF:
        v = v / f255
    elif mode == HR_REF:
        v = v / f255
        v = v * two
        v = v - one
    elif mode == HR_UNIT:
        v = v * two
        v = v - one
    assert v.dtype == np.float32
    return torch.from_numpy(v)


def dyadic_gaussian(ks, sigma, bits=12):
    """fp32 [ks, ks]: Gaussian weights rounded to multiples of 2^-bits, the centre adjusted so that the sum is exactly 1 --
    with uint8 pixels every product and partial sum is a multiple of 2^-bits not above 255 < 2^(24 - bits): exact in fp32"""
    r = ks // 2
    y, x = np.meshgrid(np.arange(ks) - r, np.arange(ks) - r, indexing="ij")
    g = np.exp(-0.5 * (x * x + 1.7 * y * y + 0.6 * x * y) / (sigma * sigma))          # (not symmetric: a transposed tap shows)
    q = np.round(g / g.sum() * (1 << bits)).astype(np.int64)
    q[r, r] += (1 << bits) - q.sum()
    assert q.sum() == 1 << bits and (q >= 0).all()
    return (q.astype(np.float64) / (1 << bits)).astype(np.float32)
