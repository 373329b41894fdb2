"""Case table, inputs, float64 references, the per-block bound and an fp32 emulation for the sweep of the Y-channel kernels
(csrc/luma.hip) past one block per image: tests/test_gpu_luma_sweep.py runs the kernels against these, and
tests/test_host_luma_sweep.py shows on the CPU that each case has the block count listed, that the emulation in the kernel's own
order is inside the bound and that three wrong variants are outside.  Test infrastructure: no product code is used here.

luma_kernel gives a block LUMA_CHUNK = 4096 consecutive cropped pixels of one image (row-major over the cropped region) and
stores partial[n * B + blk] = the sum of dY^2 over that chunk, B = ceil(h w / 4096), dY = (65.481 dr + 128.553 dg + 24.966 db) *
inv with d. the channel differences (of the 8-bit codes and inv = 1 / 255^2 with `quantize`, of the values and inv = 1 / 255
without).

The bound of a block, u = 2^-24, A = (65.481 |dr| + 128.553 |dg| + 24.966 |db|) * inv per pixel (the sum of magnitudes, not |dY|:
the three channel differences can cancel):

    sum over the block's pixels of (2 c u |dY| A + (c u A)^2)  +  24 u sum dY^2

c = 8 with `quantize`, 9 without: the three fp32 constants, the product, the two fused steps and the multiply by inv, plus one
rounding of each channel difference when the inputs are not integers.  24: the 16 fused accumulations of a thread, the 6
butterfly steps and the 2 adds over the waves."""
import functools

import numpy as np
import torch

import luma_ref

CHUNK = 4096
U = 2.0 ** -24
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# name -> (N, H, W, shave, B)
CASES = {
    "ragged": (3, 70, 121, 3, 2),       # 64 x 115 = 7360: a row of 115 straddles pixel 4096; the last block holds 3264
    "full": (1, 64, 64, 0, 1),          # 4096: a block with no guard firing
    "plus-one": (1, 17, 241, 0, 2),     # 4097: a last block of one pixel
    "two-full": (2, 64, 128, 0, 2),     # 8192: n / B with B > 1 and no tail
    "many": (18, 70, 121, 3, 2),        # N > 16: waves 0 and 1 of the finalize take a second image
    "long": (2, 515, 523, 1, 66),       # 513 x 521 = 267273: B > 64, lanes 0 and 1 of the finalize take a second partial
}


def c_of(quantize):
    return 8 if quantize else 9


def region(name):
    n, H, W, s, B = CASES[name]
    return H - 2 * s, W - 2 * s


def blocks_of(hw):
    return -(-hw // CHUNK)


@functools.lru_cache(maxsize=None)
def inputs(name, dp="fp32", dt="fp32"):
    """(preds, target) on the CPU, read only: target uniform in [0, 1], preds = target + N(0, 0.05) left unclamped."""
    n, H, W, s, _ = CASES[name]
    g = torch.Generator().manual_seed(4000 + 100 * n + H + W)
    t = torch.rand(n, 3, H, W, generator=g)
    p = t + 0.05 * torch.randn(n, 3, H, W, generator=g)
    assert p.min().item() < 0 and p.max().item() > 1
    return p.to(DTYPES[dp]), t.to(DTYPES[dt])


def channel_differences(p, t, shave, quantize):
    """float64 [N, 3, h w]: q(p) - q(t) over the cropped region in row-major order, in unit scale."""
    d = luma_ref.crop(luma_ref.quantise(p, quantize), shave) - luma_ref.crop(luma_ref.quantise(t, quantize), shave)
    return d.reshape(d.shape[0], 3, -1)


def _per_block(v):
    """float64 [N, hw] -> [N * B]: sums over chunks of 4096 (the last one short)."""
    n, hw = v.shape
    B = blocks_of(hw)
    padded = torch.zeros(n, B * CHUNK, dtype=torch.float64)
    padded[:, :hw] = v
    return padded.view(n * B, CHUNK).sum(dim=1)


def table_and_bound(p, t, shave, quantize):
    """(float64 [N * B] partial table, float64 [N * B] bound) of the module docstring.  dY is luma_ref.rgb_to_y(p) -
    luma_ref.rgb_to_y(t); A comes from the channel differences."""
    dy = (luma_ref.rgb_to_y(p, shave, quantize) - luma_ref.rgb_to_y(t, shave, quantize)).reshape(p.shape[0], -1)
    d = channel_differences(p, t, shave, quantize).abs()
    a = (luma_ref.WEIGHTS[0] * d[:, 0] + luma_ref.WEIGHTS[1] * d[:, 1] + luma_ref.WEIGHTS[2] * d[:, 2]) / 255.0
    c = c_of(quantize)
    table = _per_block(dy * dy)
    bound = _per_block(2 * c * U * dy.abs() * a + (c * U * a) ** 2) + 24 * U * table
    return table, bound


@functools.lru_cache(maxsize=None)
def reference(name, quantize, dp="fp32", dt="fp32"):
    """table_and_bound of inputs(name, dp, dt): computed once per case, shared, never modified."""
    p, t = inputs(name, dp, dt)
    return table_and_bound(p, t, CASES[name][3], quantize)


def worst_ratio(got, want, bound):
    """Largest |got - want| / bound; a block whose bound is 0 (identical pixels) has to be exact."""
    err = (got.double() - want).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


# ----------------------------------------------------------------------------- fp32 in the kernel's own order
F = np.float32
W_R, W_G, W_B = F(65.481), F(128.553), F(24.966)


def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 values is exact in float64; the sum is rounded to float64 and then to
    fp32 (a double rounding that differs from one rounding in rare last-bit ties, 2^-29 of the time)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def levels(x, quantize):
    """luma_level: rintf(fminf(fmaxf(x, 0), 1) * 255.0f) or x, as float32 numpy of the cropped region flattened."""
    x = x.float().numpy()
    return np.rint(np.clip(x, F(0), F(1)) * F(255)).astype(F) if quantize else x


def _flat(x, shave):
    c = luma_ref.crop(x, shave)
    return c.reshape(c.shape[0], 3, -1)


def emulate_dy(p, t, shave, quantize, subtract_lumas=False):
    """float32 [N, hw]: the kernel's dY per cropped pixel.  subtract_lumas: the WRONG variant Y(p) - Y(t), each luma formed as
    luma_y does and the difference taken after."""
    lp, lt = levels(_flat(p, shave), quantize), levels(_flat(t, shave), quantize)
    dot = lambda r, g, b: _fma(np.broadcast_to(W_B, b.shape), b, _fma(np.broadcast_to(W_G, g.shape), g, W_R * r))
    if subtract_lumas:
        def y(l):
            v = dot(l[:, 0], l[:, 1], l[:, 2])
            if quantize:
                v = v / F(255)
            return (F(16) + v) / F(255)
        return y(lp) - y(lt)
    inv = F(1) / (F(255) * F(255)) if quantize else F(1) / F(255)
    return dot(lp[:, 0] - lt[:, 0], lp[:, 1] - lt[:, 1], lp[:, 2] - lt[:, 2]) * inv


def emulate_blocks(d, guard=True):
    """float32 dY [N, hw] -> float32 [N * B]: thread t of a block accumulates pixels k * 256 + t (k = 0 .. 15) with fmaf, the
    64 lanes of a wave fold by the xor butterfly (32, 16, .., 1), thread 0 stores (r0 + r1) + (r2 + r3).  guard=False: the WRONG
    variant whose last block runs on past the image's h w pixels into the next image's (the last image has none to run into
    and keeps its guard)."""
    n, hw = d.shape
    B = blocks_of(hw)
    padded = np.zeros((n, B * CHUNK), dtype=F)
    padded[:, :hw] = d
    if not guard:
        tail = B * CHUNK - hw
        padded[:-1, hw:] = d[1:, :tail]
    v = padded.reshape(n * B, CHUNK // 256, 256)
    acc = np.zeros((n * B, 256), dtype=F)
    for k in range(CHUNK // 256):
        acc = _fma(v[:, k], v[:, k], acc)
    acc = acc.reshape(n * B, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    r = acc[:, :, 0]
    return torch.from_numpy((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3]))


def sequential_blocks(d):
    """float32 dY [N, hw] -> float32 [N * B]: one fp32 accumulator running over the chunk in pixel order (no kernel does this;
    it shows how much room the bound leaves)."""
    n, hw = d.shape
    B = blocks_of(hw)
    padded = np.zeros((n, B * CHUNK), dtype=F)
    padded[:, :hw] = d
    v = padded.reshape(n * B, CHUNK)
    acc = np.zeros(n * B, dtype=F)
    for k in range(CHUNK):
        acc = _fma(v[:, k], v[:, k], acc)
    return torch.from_numpy(acc)


# ----------------------------------------------------------------------------- one 8-bit step of one green value
STEP_POSITIONS = (0, CHUNK - 1, CHUNK, 64 * CHUNK, 65 * CHUNK, None)      # cropped flat indices in `long`; None: h w - 1


@functools.lru_cache(maxsize=None)
def one_step_pair(dtype_name):
    """(preds, target, closed-form PSNR-Y) for shape `long` with six images, read only: preds equal the target except one green
    value, code 10 against 11, at cropped flat index STEP_POSITIONS[n] of image n."""
    _, H, W, s, B = CASES["long"]
    h, w = H - 2 * s, W - 2 * s
    g = torch.Generator().manual_seed(77)
    t = torch.rand(6, 3, H, W, generator=g).to(DTYPES[dtype_name])
    p = t.clone()
    for n, i in enumerate(STEP_POSITIONS):
        i = h * w - 1 if i is None else i
        y, x = i // w + s, i % w + s
        t[n, 1, y, x] = 10.0 / 255.0
        p[n, 1, y, x] = 11.0 / 255.0
    closed = 10.0 * np.log10(h * w * 255.0 ** 4 / 128.553 ** 2)
    return p, t, closed


# ----------------------------------------------------------------------------- the finalize on a synthetic table
FIN = (35, 730, 730, 0, 131)          # N, H, W, shave, B: 532900 pixels


@functools.lru_cache(maxsize=None)
def finalize_table(with_zero_image):
    """(float32 [N * B] partials, float64 [N] PSNR) for FIN: integers * 2^-20 below 2^24, so every partial is an fp32 value and
    the float64 sum of an image's 131 is exact in any order.  with_zero_image: image 20's partials are all zero (+inf)."""
    n, H, W, s, B = FIN
    g = torch.Generator().manual_seed(5)
    ints = torch.randint(1, 1 << 20, (n, B), generator=g, dtype=torch.int64)
    if with_zero_image:
        ints[20] = 0
    table = (ints.double() * 2.0 ** -20)
    assert bool((table.float().double() == table).all())
    sse = ints.sum(dim=1).double() * 2.0 ** -20                        # exact: below 2^53
    count = float((H - 2 * s) * (W - 2 * s))
    psnr = torch.tensor([10.0 * np.log10(count / v) if v > 0 else np.inf for v in sse.tolist()], dtype=torch.float64)
    return table.float().reshape(-1), psnr
