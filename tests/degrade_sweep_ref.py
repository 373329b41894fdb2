"""Kernels, images, case tables and wrong variants for the sweep of the blind-degradation kernel (csrc/degrade.hip) over every
scale: tests/test_gpu_degrade_sweep.py launches both entry points against tests/degrade_ref.py on these, and
tests/test_host_degrade_sweep.py shows on the CPU that the data is in the regime claimed and that each wrong variant differs from
the yardstick on it.  The yardstick itself (blur, finish, scale_f32) is tests/degrade_ref.py's and is not restated.

THE EXACT REGIME.  Weights are multiples of 2^-12 with sum |k| <= 8 and pixels are uint8, so every product and every partial sum,
in any order, is a multiple of 2^-12 of magnitude at most 8 * 255 = 2040 < 2^11: 23 bits, which fp32 holds.  The accumulator does
not depend on rounding, clipping and rintf act on exact values, and the comparison is bit for bit through degrade_ref.scale_f32.

THE KERNELS.  What the other degrade tests feed the kernel is point-symmetric (k[i][j] == k[ks-1-i][ks-1-j]), so taps walked
backwards would pass them.  Here:
  unsymmetric(ks)   non-negative, random, sums to exactly 1, no symmetry at all
  signed(ks)        seven heavy taps of alternating sign (+-0.73 .. 0.98) over small signed noise, sum |k| <= 8: on random pixels
                    the outputs have a spread of about 170 grey levels round 110 and leave 0..255 at both ends
  two_tap()         ks = 3, weights 1/2 at (1, 0) and (1, 2): half of the outputs are exact .5 ties"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import degrade_ref

BITS = 12
ONE = 1 << BITS
SCALES = list(range(1, 9))
KS = list(range(1, 22, 2))
TW = 16                                 # LR columns of a tile


def tile_rows(s):
    return 16 if s <= 4 else 8


def offsets(s):
    return sorted({0, s // 2, s - 1})


def image_shape(s):
    return 20 * s + 3, 35 * s + 5


def grid(shape, s, offset):
    return (shape[0] - offset + s - 1) // s, (shape[1] - offset + s - 1) // s


@functools.lru_cache(maxsize=None)
def image(s):
    """uint8 [20 s + 3, 35 s + 5, 3], read only: the one image of scale s."""
    h, w = image_shape(s)
    return np.random.RandomState(700 + s).randint(0, 256, (h, w, 3), dtype=np.uint8)


def small_size(ks):
    return ks // 2 + 1                  # the smallest image both entry points accept: ks / 2 < min(H, W)


@functools.lru_cache(maxsize=None)
def small_image(ks):
    n = small_size(ks)
    return np.random.RandomState(900 + ks).randint(0, 256, (n, n, 3), dtype=np.uint8)


def small_offsets(ks, s):
    """The sweep's offsets that leave the LR grid of the smallest image non-empty."""
    return [o for o in offsets(s) if o < small_size(ks)]


# ----------------------------------------------------------------------------- kernels
def _f32(q):
    k = (q.astype(np.float64) / ONE).astype(np.float32)
    assert np.array_equal(k.astype(np.float64) * ONE, q)
    return k


@functools.lru_cache(maxsize=None)
def unsymmetric(ks):
    rng = np.random.RandomState(1000 + ks)
    w = rng.rand(ks, ks) ** 3
    q = np.floor(w / w.sum() * ONE).astype(np.int64)
    q[0, ks - 1] += ONE - q.sum()                       # the remainder on a corner tap
    return _f32(q)


HEAVY = 7


@functools.lru_cache(maxsize=None)
def signed(ks):
    if ks == 1:
        return _f32(np.array([[7 * ONE // 4]], dtype=np.int64))          # one tap: 1.75 (clips at the top only)
    rng = np.random.RandomState(2000 + ks)
    q = rng.randint(-8, 9, (ks, ks)).astype(np.int64)
    pos = rng.choice(ks * ks, HEAVY, replace=False)
    mag = rng.randint(3000, 4001, HEAVY)
    for n, (at, m) in enumerate(zip(pos, mag)):
        q[at // ks, at % ks] = m if n % 2 == 0 else -m
    return _f32(q)


def claims_both_clips(ks):
    return ks >= 3


def two_tap():
    q = np.zeros((3, 3), dtype=np.int64)
    q[1, 0] = q[1, 2] = ONE // 2
    return _f32(q)


FAMILIES = {"unsymmetric": unsymmetric, "signed": signed}


# ----------------------------------------------------------------------------- the yardstick, once per (image, kernel)
@functools.lru_cache(maxsize=None)
def full_blur(which, key, family, ks):
    """float64 [3, H, W]: degrade_ref.blur at full resolution of image(key) (which == "sweep") or small_image(key) ("small") under
    the family's kernel of size ks ("two_tap": ks is 3).  Computed once, read only; subsampled per (s, offset) by lr()."""
    img = image(key) if which == "sweep" else small_image(key)
    k = two_tap() if family == "two_tap" else FAMILIES[family](ks)
    return degrade_ref.blur(img, k, 1, 0)


def lr(full, s, offset, quantise):
    """float64 [3, h, w] in 0..255 units: the sampled, clipped and (optionally) rounded result."""
    return degrade_ref.finish(full[:, offset::s, offset::s], quantise=quantise)


def as_f32(v255):
    """what dsr_degrade_batch_u8 stores in mode UNIT: fp32 [3, h, w]"""
    return degrade_ref.scale_f32(v255, degrade_ref.UNIT)


def as_u8(v255):
    """what dsr_degrade_image_u8 stores: uint8 [h, w, 3] of an already rounded result"""
    assert torch.equal(v255, torch.round(v255))
    return v255.permute(1, 2, 0).to(torch.uint8).contiguous()


def clear():
    for f in (image, small_image, unsymmetric, signed, full_blur):
        f.cache_clear()


# ----------------------------------------------------------------------------- fp32 in tap order, and the wrong variants
def blur_f32_tap_order(img, kernel):
    """float32 [3, H, W]: one fp32 accumulator per output, taps in row-major order, the product and the sum each rounded to
    fp32 (in the exact regime neither rounds)."""
    x = np.asarray(img).transpose(2, 0, 1).astype(np.float32)
    ks = kernel.shape[0]
    r = ks // 2
    xp = np.pad(x, ((0, 0), (r, r), (r, r)), mode="reflect") if r else x
    h, w = x.shape[1:]
    acc = np.zeros_like(x)
    for i in range(ks):
        for j in range(ks):
            acc = acc + kernel[i, j] * xp[:, i:i + h, j:j + w]
    assert acc.dtype == np.float32
    return torch.from_numpy(acc)


def blur_edge_repeating(img, kernel):
    """The WRONG reflection that repeats the edge pixel (-1 -> 0, H -> H - 1: numpy's 'symmetric')."""
    x = np.asarray(img).transpose(2, 0, 1).astype(np.float64)
    r = kernel.shape[0] // 2
    xp = torch.from_numpy(np.pad(x, ((0, 0), (r, r), (r, r)), mode="symmetric"))[None]
    wt = torch.from_numpy(kernel.astype(np.float64))[None, None].expand(3, 1, -1, -1).contiguous()
    return F.conv2d(xp, wt, groups=3)[0]


def round_half_up(v):
    return torch.floor(v + 0.5)
