"""Float64 references, operand generators and case tables of the metric-kernel sweep (csrc/metrics.hip through the raw C ABI:
test_gpu_metrics_sweep.py on the MI355X, test_host_metrics_sweep.py on the CPU).  Test infrastructure, written from the contracts
in include/dsr_hip.h; nothing is imported from the package.  ssim_ref.py / msssim_ref.py supply the window and the maps.

What is here:
  tile_sums            per-tile sums of a window-position map in the kernels' block order, with the tile's position count
  one_scale_loss       one scale of multi-scale SSIM as a scalar whose autograd is the reference of dsr_(ms)ssim_bwd_f32
  psnr_partials        per-chunk SSE and ordered min / max keys; metric_key / metric_unkey; both finalise modes and the state
  combine              dsr_msssim_combine: value, vals, factors
  the case tables      shapes, operand generators and the launcher predicates (which instantiation a case takes)
  the floors           what the float32 CPU restatement of the same operation deviates from float64 on the same operands:
                       F(n) per tile size for the forward sums, relative-L2 and per-pixel floors for the gradients

The constants below restate csrc/metrics.hip; test_host_metrics_sweep.py reads them from that file as text and compares."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import msssim_ref
import ssim_ref

F64, F32 = torch.float64, torch.float32
SSIM_K = 11
SF_TH, SF_TW = 16, 64            # ssim_img_kernel<CS>: window positions per block
SB_T = 32                        # ssim_bwd_kernel<MS>: gradient pixels per block (square)
PSNR_CHUNK = 16384               # psnr_stats_kernel<V4>: elements per block
FIN_WAVES, FIN_LANES = 16, 64    # the one-block finalisers: images stride the waves, blocks of an image stride the lanes
COMBINE_THREADS = 256            # msssim_combine_kernel: images stride the threads
ACC_LANES = 64                   # metric_accumulate_kernel
C1, C2 = 0.01 ** 2, 0.03 ** 2    # data_range 1
EPS32 = 2.0 ** -24
MARGIN = 4                       # the project's margin over a measured floor (test_gpu_metrics.py)
REL_FLOOR = 1e-6                 # ... and the least floor it accepts


def f32(x):
    """The float64 value of x rounded to float32 (how a float argument of the C ABI arrives)."""
    return float(np.float32(x))


def q32(t):
    """float64 tensor rounded to float32 and back: the operand the kernel actually sees."""
    return t.to(F32).to(F64)


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor or array in, same out); the subnormal spacing below the normals."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.exp2(np.maximum(e, -126.0) - 23.0)


# ================================================================================ forward: tiles
def tile_grid(oh, ow, th, tw):
    return -(-oh // th), -(-ow // tw)


def tile_sums(m, th, tw):
    """m [N, C, OH, OW] -> (sums, counts), each [N * C * tiles_y * tiles_x] in the kernels' block order: plane-major, then tile
    row, then tile column.  The sums are taken in m's dtype; counts are int64."""
    n, c, oh, ow = m.shape
    ty, tx = tile_grid(oh, ow, th, tw)
    p = F.pad(m, (0, tx * tw - ow, 0, ty * th - oh))
    s = p.reshape(n * c, ty, th, tx, tw).sum(dim=(2, 4)).reshape(-1)
    one = F.pad(torch.ones(1, 1, oh, ow, dtype=F64), (0, tx * tw - ow, 0, ty * th - oh))
    cnt = one.reshape(1, ty, th, tx, tw).sum(dim=(2, 4)).to(torch.int64).expand(n * c, ty, tx).reshape(-1)
    return s, cnt


def tile_counts(shape, th, tw):
    n, c, h, w = shape
    return tile_sums(torch.zeros(n, c, h - SSIM_K + 1, w - SSIM_K + 1, dtype=F64), th, tw)[1]


def blocks_per_image(shape, th, tw):
    _, c, h, w = shape
    ty, tx = tile_grid(h - SSIM_K + 1, w - SSIM_K + 1, th, tw)
    return c * ty * tx


AMPLITUDES = (0.05, 0.3, 1.0)
FWD_SHAPES = [(1, 1, 11, 11), (2, 3, 27, 75), (2, 3, 43, 139), (1, 3, 91, 203), (17, 1, 12, 76), (64, 1, 11, 11)]


@functools.lru_cache(maxsize=None)
def fwd_case(shape):
    """(a, b) float64, already rounded to float32: msssim_ref.textured_pair with a different noise amplitude per image (0.05, 0.3,
    1.0 rotating, so a plane mix-up shows).  (64, 1, 11, 11) is cut from ONE textured 88 x 88 image, eight by eight: each image
    has one window position, so each partial is one SSIM value."""
    n, c, h, w = shape
    seed = 1000 * h + w + n
    if shape == (64, 1, 11, 11):
        p, t = msssim_ref.textured_pair((1, 1, 88, 88), 0.3, seed)
        cut = lambda x: x.reshape(8, 11, 8, 11).permute(0, 2, 1, 3).reshape(64, 1, 11, 11).contiguous()
        return q32(cut(p)), q32(cut(t))
    amp = [AMPLITUDES[(i + h) % 3] for i in range(n)]
    p, t = msssim_ref.textured_pair(shape, amp, seed)
    return q32(p), q32(t)


def fwd_maps(a, b):
    """(ssim_map, cs_map) in a's dtype."""
    return msssim_ref.ssim_cs_maps(a, b)


@functools.lru_cache(maxsize=None)
def fwd_reference(shape, th, tw):
    """dict: sim / cs = float64 tile sums, sim32 / cs32 = the float32 CPU restatement's, cnt = positions per tile."""
    a, b = fwd_case(shape)
    s64, q64 = fwd_maps(a, b)
    s32, q32_ = fwd_maps(a.to(F32), b.to(F32))
    sim, cnt = tile_sums(s64, th, tw)
    return {"sim": sim, "cs": tile_sums(q64, th, tw)[0], "cnt": cnt,
            "sim32": tile_sums(s32, th, tw)[0].to(F64), "cs32": tile_sums(q32_, th, tw)[0].to(F64)}


@functools.lru_cache(maxsize=None)
def fwd_floor(th, tw):
    """F(n): the largest |sum32 - sum64| over all tiles with n positions of the sweep of that tile size (every shape, the SSIM
    and the contrast-structure sums), n -> F(n)."""
    out = {}
    for shape in FWD_SHAPES:
        r = fwd_reference(shape, th, tw)
        for kind in ("sim", "cs"):
            d = (r[kind + "32"] - r[kind]).abs()
            for n in r["cnt"].unique().tolist():
                out[n] = max(out.get(n, 0.0), float(d[r["cnt"] == n].max()))
    return out


def fwd_bar(n, th, tw):
    """Bar of a tile of n positions: MARGIN x max(F(n), 1e-6 n)."""
    n = np.asarray(n)
    fl = fwd_floor(th, tw)
    f = np.array([fl[int(k)] for k in n.reshape(-1)]).reshape(n.shape)
    return MARGIN * np.maximum(f, REL_FLOOR * n)


def fold_tolerance(partials, nblk, inv_count):
    """Bound of the finaliser's float32 chain on one image: at most ceil(nblk / 64) + 6 additions and one product, each with a
    relative rounding of 2^-24 on a partial sum no larger than sum |partial| -> (nblk + 8) 2^-24 sum |partial| inv_count."""
    return (nblk + 8) * EPS32 * float(np.abs(partials).sum()) * inv_count


def total_tolerance(partials, n, nblk, inv_count, scale, result):
    """Bound of `total` = scale sum_n per_image[n] (+ what it held): every per_image carries its fold_tolerance, the N values
    are added in at most ceil(N / 16) + 16 float32 additions on partial sums no larger than sum |per_image|, then one product
    and (accumulate) one addition, each a relative 2^-24."""
    mag = float(np.abs(partials).sum()) * inv_count
    chain = (nblk + 8) + (-(-n // FIN_WAVES) + FIN_WAVES + 1)
    return chain * EPS32 * mag * abs(scale) + EPS32 * abs(result)


def impulse_pixels(shape, th, tw):
    """(y, x) of the impulse cases: both image corners, and -- where the image has an interior tile corner -- the four pixels
    around the window position (th, tw) that starts tile (1, 1)."""
    _, _, h, w = shape
    px = [(0, 0), (h - 1, w - 1)]
    if h - SSIM_K + 1 > th and w - SSIM_K + 1 > tw:
        px += [(th - 1, tw - 1), (th - 1, tw), (th, tw - 1), (th, tw)]
    return px


def impulse_case(shape, y, x, amount=0.25):
    """(a, b, plane): b = a except pixel (y, x) of the LAST plane, which is a + amount."""
    a = fwd_case(shape)[1].clone()
    b = a.clone()
    b[-1, -1, y, x] += amount
    return a, q32(b), shape[0] * shape[1] - 1


def impulse_tiles(shape, y, x, th, tw):
    """bool [blocks]: the tiles of the last plane that hold a window position covering pixel (y, x) (positions y-10 .. y by
    x-10 .. x inside the image); every other tile sees identical windows."""
    n, c, h, w = shape
    m = torch.zeros(n, c, h - SSIM_K + 1, w - SSIM_K + 1, dtype=F64)
    m[-1, -1, max(y - SSIM_K + 1, 0):y + 1, max(x - SSIM_K + 1, 0):x + 1] = 1.0
    return tile_sums(m, th, tw)[0] > 0


# ================================================================================ backward
def one_scale_loss(a, b, g, w_sim=None, w_cs=None, coarse_a=None, coarse_b=None):
    """sum_n g[n] (w_sim[n] mean ssim_n + w_cs[n] mean cs_n) + <coarse_a, avg_pool2d(a, 2)> + <coarse_b, avg_pool2d(b, 2)>, in
    a's dtype (a null weight array is 0, a null coarse gradient no term)."""
    sim, cs = msssim_ref.ssim_cs_maps(a, b, 1.0)
    loss = a.new_zeros(())
    if w_sim is not None:
        loss = loss + (g.to(a.dtype) * w_sim.to(a.dtype) * sim.mean(dim=(1, 2, 3))).sum()
    if w_cs is not None:
        loss = loss + (g.to(a.dtype) * w_cs.to(a.dtype) * cs.mean(dim=(1, 2, 3))).sum()
    if coarse_a is not None:
        loss = loss + (coarse_a.to(a.dtype) * F.avg_pool2d(a, 2)).sum()
    if coarse_b is not None:
        loss = loss + (coarse_b.to(a.dtype) * F.avg_pool2d(b, 2)).sum()
    return loss


def one_scale_grads(a, b, which, g, w_sim=None, w_cs=None, coarse_a=None, coarse_b=None, dtype=F64):
    """(grad_a, grad_b) of one_scale_loss by autograd in `dtype` (None for an image `which` does not ask for: bit 0 a, bit 1 b)."""
    x = a.to(dtype).clone().requires_grad_(bool(which & 1))
    y = b.to(dtype).clone().requires_grad_(bool(which & 2))
    one_scale_loss(x, y, g, w_sim, w_cs, coarse_a, coarse_b).backward()
    return x.grad, y.grad


BWD_SHAPES = [(1, 1, 11, 11), (1, 2, 33, 43), (2, 1, 12, 65), (1, 3, 97, 33), (2, 3, 64, 80)]
WHICH = (1, 2, 3)
WEIGHTS = ("sim", "cs", "both")
COARSE = ("none", "both", "one")


def bwd_case(shape):
    """(a, b, g, w_sim, w_cs, coarse_a, coarse_b), float64 already rounded to float32.  g differs per image and takes both signs
    (over the table, for N = 1); the weights differ per image too."""
    n, c, h, w = shape
    a, b = msssim_ref.textured_pair(shape, [AMPLITUDES[(i + w) % 3] for i in range(n)], 77 * h + w)
    gen = torch.Generator().manual_seed(h * w + n)
    g = torch.tensor([(-1.0) ** (i + h) * (0.75 + 0.5 * i) for i in range(n)], dtype=F64)
    w_sim = torch.tensor([0.6 + 0.25 * i for i in range(n)], dtype=F64)
    w_cs = torch.tensor([-0.4 + 0.7 * i for i in range(n)], dtype=F64)
    # a coarse gradient of the size the next scale's SSIM gradient has (1e-3 .. 1e-2 per pixel)
    ca = (torch.rand(n, c, h // 2, w // 2, generator=gen, dtype=F64) - 0.5) * 1e-2
    cb = (torch.rand(n, c, h // 2, w // 2, generator=gen, dtype=F64) - 0.5) * 1e-2
    return tuple(q32(t) for t in (a, b, g, w_sim, w_cs, ca, cb))


def bwd_args(shape, which, weights, coarse):
    """The operands one case hands to the kernel and to one_scale_grads: (a, b, g, w_sim, w_cs, coarse_a, coarse_b), nulls as
    None.  coarse 'one': only the first image `which` asks for gets a coarse gradient."""
    a, b, g, ws, wc, ca, cb = bwd_case(shape)
    ws = ws if weights in ("sim", "both") else None
    wc = wc if weights in ("cs", "both") else None
    if coarse == "none":
        ca = cb = None
    else:
        if not which & 1 or (coarse == "one" and which == 3 and shape[2] % 2):
            ca = None
        if not which & 2 or (coarse == "one" and which == 3 and not shape[2] % 2):
            cb = None
    return a, b, g, ws, wc, ca, cb


def ms_cases():
    """(shape, which, weights, coarse) of the multi-scale backward; 'one' differs from 'both' only where both gradients are
    asked for."""
    return [(s, wh, wt, co) for s in BWD_SHAPES for wh in WHICH for wt in WEIGHTS for co in COARSE if not (co == "one" and wh != 3)]


def rel_l2(got, ref):
    return float((got.to(F64) - ref).norm() / ref.norm())


def rel_max(got, ref):
    """The largest per-pixel error over the largest reference magnitude."""
    return float((got.to(F64) - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def bwd_reference(shape, which, weights, coarse, impulse=None):
    """[(ref64, floor_l2, floor_max) or None for grad_a, grad_b]: float64 autograd of one_scale_loss, and what float32 CPU
    autograd of the same deviates from it.  weights None: the plain SSIM backward (w_sim = 1).  impulse (y, x): b = a except
    that pixel of the last plane (+0.25), no coarse terms."""
    a, b, g, ws, wc, ca, cb = bwd_operands(shape, which, weights, coarse, impulse)
    r = one_scale_grads(a, b, which, g, ws, wc, ca, cb, F64)
    f = one_scale_grads(a, b, which, g, ws, wc, ca, cb, F32)
    return [None if x is None else (x, rel_l2(y, x), rel_max(y, x)) for x, y in zip(r, f)]


def bwd_operands(shape, which, weights, coarse, impulse=None):
    a, b, g, ws, wc, ca, cb = bwd_args(shape, which, weights or "sim", coarse)
    if weights is None:
        ws = torch.ones_like(g)
    if impulse is not None:
        a = b.clone()
        b = b.clone()
        b[-1, -1, impulse[0], impulse[1]] += 0.25
        b = q32(b)
    return a, b, g, ws, wc, ca, cb


def bwd_bars(floor_l2, floor_max):
    return MARGIN * max(floor_l2, REL_FLOOR), MARGIN * max(floor_max, REL_FLOOR)


def far_from_impulse(shape, y, x):
    """bool [N, C, H, W]: pixels no window position shares with pixel (y, x) of the last plane -- everything outside the 21 x 21
    pixels around it, and every other plane.  With b = a elsewhere the float64 gradient is zero there (SSIM is at its maximum)."""
    n, c, h, w = shape
    far = torch.ones(shape, dtype=torch.bool)
    far[-1, -1, max(y - SSIM_K + 1, 0):y + SSIM_K, max(x - SSIM_K + 1, 0):x + SSIM_K] = False
    return far


def bwd_impulse_pixels(shape):
    _, _, h, w = shape
    px = [(0, 0), (h - 1, w - 1)]
    if h > SB_T and w > SB_T:
        px += [(SB_T - 1, SB_T - 1), (SB_T - 1, SB_T), (SB_T, SB_T - 1), (SB_T, SB_T)]
    return px


def bwd_nm(which):
    """Coefficient maps the backward carries: 4 when both gradients are asked for, else 3."""
    return 4 if which == 3 else 3


# ================================================================================ PSNR
def metric_key(x):
    """float32 array -> uint32 keys of the same order (f >= 0: bits | 0x80000000, f < 0: ~bits; -0 sorts below +0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32).reshape(np.shape(x))


def metric_unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


PSNR_E = (1, 3, 4, 5, 16380, 16383, 16384, 16385, 16388, 32772, 65 * 16384 + 4)
PSNR_N = (1, 2, 17, 33)
PSNR_MAX_ELEMENTS = 1_200_000
SPECIALS = np.array([-0.0, 0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), -3.0, -15.0, 7.0], dtype=np.float32)


def psnr_cases():
    """(N, E, offset): every E with every N that keeps N E within about 1 M elements (the 65-chunk E runs with N = 1), aligned;
    and with both inputs offset by one float wherever E % 4 == 0, which takes the scalar form on a V4 shape."""
    out = []
    for e in PSNR_E:
        for n in PSNR_N:
            if n * e <= PSNR_MAX_ELEMENTS:
                out.append((n, e, 0))
                if e % 4 == 0:
                    out.append((n, e, 1))
    return out


def psnr_form(e, offset):
    """'v4' or 'scalar': the launcher's choice for torch allocations (16-byte aligned) shifted by `offset` floats."""
    return "v4" if e % 4 == 0 and offset % 4 == 0 else "scalar"


def psnr_case(n, e, shift=0):
    """(preds, target) float32 [n, e].  The target is integer-valued in [-20, 20] (+ shift) with the SPECIALS (signed zeros,
    subnormals, negatives) planted at the start, the end and across every chunk edge of image n - 1; the prediction is the
    target plus an integer d, |d| <= 15, d = 0 at the subnormals (so every d and d^2 is an exact integer) and d != 0 at
    element 0 of every image (no image has SSE 0).  Any 16384-element chunk sums to at most 15^2 16384 < 2^24."""
    rng = np.random.default_rng(1_000_003 * n + e + 17 * shift)
    t = rng.integers(-20, 21, size=(n, e)).astype(np.float32) + np.float32(shift)
    d = rng.integers(-15, 16, size=(n, e)).astype(np.float32)
    d[:, 0] = np.where(d[:, 0] == 0, 15.0, d[:, 0])
    k = len(SPECIALS)
    if e > 2 * k + 2:
        spots = [1, e - k] + [c - k // 2 for c in range(PSNR_CHUNK, e - k, PSNR_CHUNK)]
        for s in spots:
            t[n - 1, s:s + k] = SPECIALS
    elif e > 1:
        m = min(k, e - 1)
        t[n - 1, 1:1 + m] = SPECIALS[:m]
    sub = (t != 0) & (np.abs(t) < 2.0 ** -126)
    d[sub] = 0.0
    p = (t + d).astype(np.float32)
    return p, t


def psnr_partials(p, t):
    """(sse float64 [n * B], keys uint32 [n * B, 2]) per block, blocks of an image consecutive, B = ceil(E / PSNR_CHUNK)."""
    n, e = t.shape
    nb = -(-e // PSNR_CHUNK)
    d = p.astype(np.float64) - t.astype(np.float64)
    key = metric_key(t)
    sse, keys = np.zeros((n, nb)), np.zeros((n, nb, 2), dtype=np.uint32)
    for b in range(nb):
        sl = slice(b * PSNR_CHUNK, min((b + 1) * PSNR_CHUNK, e))
        sse[:, b] = (d[:, sl] ** 2).sum(axis=1)
        keys[:, b, 0], keys[:, b, 1] = key[:, sl].min(axis=1), key[:, sl].max(axis=1)
    return sse.reshape(-1), keys.reshape(-1, 2)


def psnr_per_image(sse, n, e, data_range, log_scale):
    """float64 [n]: log_scale (2 ln range - ln(SSE_n / E)); range and log_scale as float32 carries them."""
    s = sse.reshape(n, -1).sum(axis=1)
    return f32(log_scale) * (2.0 * math.log(f32(data_range)) - np.log(s / e))


def psnr_batch(sse, keys, n, e, infer_range, data_range, log_scale):
    """(value, SSE, count, target min, target max) of the batch mode."""
    s = float(sse.sum())
    lo, hi = float(metric_unkey(keys[:, 0].min())), float(metric_unkey(keys[:, 1].max()))
    r = max(hi, 0.0) - min(lo, 0.0) if infer_range else f32(data_range)
    return f32(log_scale) * (2.0 * math.log(r) - math.log(s / (n * e))), s, float(n) * e, lo, hi


def psnr_state_after(state, batch):
    """The four-word running state after one batch-mode finalise: SSE and count added, min and max folded in."""
    _, s, cnt, lo, hi = batch
    return [state[0] + s, state[1] + cnt, min(state[2], lo), max(state[3], hi)]


def psnr_of_state(state, infer_range, data_range, log_scale):
    r = state[3] - state[2] if infer_range else f32(data_range)
    return f32(log_scale) * (2.0 * math.log(r) - math.log(state[0] / state[1]))


LOG_SCALES = (10.0 / math.log(10.0), 10.0 / math.log(2.0))
ACC_N = (1, 63, 64, 65, 130)


def acc_case(n):
    """float32 [n], multiples of 1/1024 in [-8, 8]: every partial sum is exact in double, in any order."""
    rng = np.random.default_rng(n)
    return (rng.integers(-8192, 8193, size=n) / 1024.0).astype(np.float32)


# ================================================================================ 2 x 2 mean pool of a pair
POOL_CASES = [(1, 2, 2, 0), (3, 5, 6, 0), (2, 7, 8, 0), (2, 9, 12, 0), (2, 8, 12, 1), (1, 4, 4, 0), (5, 13, 1028, 0)]


def pool_form(w, offset):
    return "v4" if w % 4 == 0 and offset % 4 == 0 else "scalar"


def pool_case(planes, h, w):
    """(in1, in2) float64 [planes, h, w], different from each other: multiples of 1/16 in [-64, 64].  Any four-term sum is a
    multiple of 1/16 below 2^9 and its quarter a multiple of 1/64: both exact in float32, in any order."""
    g = torch.Generator().manual_seed(planes * 10007 + h * 101 + w)
    mk = lambda: torch.randint(-1024, 1025, (planes, h, w), generator=g).to(F64) / 16.0
    return mk(), mk()


def pool_ref(x):
    return F.avg_pool2d(x[None], 2)[0]


# ================================================================================ combine
COMBINE_N = (1, 255, 256, 257, 600)
COMBINE_L = (1, 3, 5, 8)
BETAS8 = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333, 0.05, 0.5, 1.0)
NORMALIZE = (0, 1, 2)


def combine_case(n, levels):
    """raw float32 [L, n] in (-0.6, 1]: mostly positive, with negatives, exact +0 and -0 planted (image 0 of n > 1 stays
    positive in every scale; for n = 1 scale 0 is 0 where L > 1)."""
    rng = np.random.default_rng(100 * n + levels)
    raw = rng.uniform(0.15, 1.0, size=(levels, n)).astype(np.float32)
    for i in range(1, n):
        s = (i * 7) % levels
        if i % 5 == 1:
            raw[s, i] = 0.0
        elif i % 5 == 2:
            raw[s, i] = np.float32(-0.6 * rng.uniform(0.1, 1.0))
        elif i % 5 == 3:
            raw[s, i] = -0.0
    if n == 1 and levels > 1:
        raw[0, 0] = 0.0
    return raw


def combine(raw, betas, normalize):
    """(per_image float64 [N], vals float32 [L, N], factors float64 [L, N]) of dsr_msssim_combine.  vals are float32 operations
    (max(raw, 0), (raw + 1) / 2: one rounding each, the same one); the product and the factors are float64 of those.
    Stated rule, relu: 0 where v <= 0 -- the image's value is 0 there and so are all its factors.  Without that rule the
    arithmetic is what it is: normalize 0 has NaN for a negative value (pow of a negative base) and 0 / 0 = NaN factors at 0."""
    raw = np.asarray(raw, dtype=np.float32)
    if normalize == 1:
        vals = np.maximum(raw, np.float32(0.0))
    elif normalize == 2:
        vals = ((raw + np.float32(1.0)) * np.float32(0.5)).astype(np.float32)
    else:
        vals = raw.copy()
    v = vals.astype(np.float64)
    bt = np.array([f32(b) for b in betas], dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        out = np.prod(np.power(v, bt), axis=0)
        fac = bt * out[None, :] / v
        if normalize == 1:
            fac = np.where(v > 0.0, fac, 0.0)
            dead = (v <= 0.0).any(axis=0)
            out = np.where(dead, 0.0, out)
            fac = np.where(dead[None, :], 0.0, fac)
        if normalize == 2:
            fac = fac * 0.5
    return out, vals, fac


def within_ulp32(got, ref, ulps=1.0):
    """got (float32 array) within `ulps` float32 ulp of ref (float64); NaN exactly where ref is NaN, +-inf where ref is."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin & ~nan], ref[~fin & ~nan]):
        return False
    return bool((np.abs(got[fin] - ref[fin]) <= ulps * ulp32(ref[fin])).all())
