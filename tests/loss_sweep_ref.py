"""Case tables, float64 / exact references and derived bounds of the loss-kernel sweep (tests/test_host_loss_sweep.py on the CPU,
tests/test_gpu_loss_sweep.py on the device): csrc/lpips.hip, csrc/featloss.hip and the loss section of csrc/pointwise.hip at the
shapes where each kernel leaves its first grid pass.  Test infrastructure: the package never imports it.

Every threshold below restates a launcher's own arithmetic (lp_grid, lpips_table, dsr_pw_reduce_blocks, feat_stream_grid,
dsr_gan_loss_blocks, the axpby grid); the tests assert each case against these AND against what the ABI reports, so a changed
cap turns a case red instead of moving it back onto the first pass."""
import functools
import struct

import torch
import torch.nn.functional as TF

import lpips_ref

MARGIN = 1024          # sentinel elements on each side of a raw buffer (as tests/test_gpu_rrdb.py)
SENTINEL = 7777.0
U32 = 2.0 ** -24       # relative error of one correctly rounded fp32 operation

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.bfloat16: 8, torch.float16: 11}             # significand bits, hidden one included
EMIN = {torch.bfloat16: -126, torch.float16: -14}         # exponent of the smallest normal number

LPIPS_GRID_ITEMS = 4096 * 256                             # lp_grid: 4096 blocks x 256 threads, grid-stride beyond
LPIPS_PIX_PER_BLOCK = 256
FEAT_STREAM_ITEMS = 2048 * 256                            # feat_stream_grid
AXPBY_ITEMS = 4096 * 256


def ulp16(ref64, dtype):
    """Spacing of the 16-bit type at |ref| (the subnormal step below the normal range)."""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** EMIN[dtype]))).clamp_min(EMIN[dtype])
    return torch.exp2(e - (MANT[dtype] - 1))


def ulp32(t64):
    """One fp32 ulp at each |value| (the rule of tests/test_gpu_ganloss.py)."""
    a = t64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def round_once(x64, dtype):
    """float64 -> storage type with ONE rounding: the value must already be exact in fp32."""
    f = x64.float()
    assert torch.equal(f.double(), x64)
    return f.to(dtype)


def worst_ratio(got64, ref64, tol):
    """Largest |got - ref| / tol; where nothing is allowed (tol == 0) the values must be equal."""
    err = (got64 - ref64).abs()
    zero = tol == 0
    assert bool((err[zero] == 0).all()), "a deviation where the allowance is zero"
    return float((err[~zero] / tol[~zero]).max()) if bool((~zero).any()) else 0.0


# ============================================================================= 1. LPIPS streaming kernels
PREP_SHAPE = (2, 727, 731)            # N pairs, H, W
POOL_SHAPE = (2, 515, 517, 64)        # N, H, W, Cp


def stem_blocks(h, w):
    """(BH, BW) of the space-to-depth stem input: the 11x11/4 pad-2 output size + 2 (lpips_sizes in csrc/lpips.hip)."""
    return (h + 4 - 11) // 4 + 3, (w + 4 - 11) // 4 + 3


def prep_items(n, h, w):
    bh, bw = stem_blocks(h, w)
    return 2 * n * bh * bw * 8, n * h * w                                    # (forward, backward) work items


def pool_items(n, h, w, cp):
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return n * oh * ow * (cp // 8), n * ((h + 1) // 2) * ((w + 1) // 2) * (cp // 8)


def lp_key(f):
    """order_key of csrc/dsr_common.h (lpips.hip's range words) on the fp32 bits of f: an unsigned key of the same order; a NaN
    lands outside [-inf, +inf]."""
    (b,) = struct.unpack("<I", struct.pack("<f", f))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


@functools.lru_cache(maxsize=None)
def prep_inputs(normalize):
    """(img1, img2) fp32 [N,3,H,W] in the accepted range, the maximum planted in img1, the minimum in img2 -- a negative one
    without `normalize` (with a -0.0 in each image as an ordinary value), -0.0 itself with it: below +0.0 in key order."""
    n, h, w = PREP_SHAPE
    g = torch.Generator().manual_seed(1000 + int(normalize))
    lo = 0.0 if normalize else -1.0
    a = torch.rand(n, 3, h, w, generator=g) * (0.98 - lo * 0.98) + lo * 0.98 + (0.01 if normalize else 0.0)
    b = torch.rand(n, 3, h, w, generator=g) * (0.98 - lo * 0.98) + lo * 0.98 + (0.01 if normalize else 0.0)
    a[1, 2, h - 1, w - 1] = 1.0                          # the maximum: last pixel of the last image of img1 (second grid pass)
    b[0, 1, 5, 7] = -0.0
    if not normalize:
        a[0, 0, 3, 3] = -0.0
        b[1, 0, h - 2, 11] = -1.0
    return a, b


def prep_range_words(normalize):
    a, b = prep_inputs(normalize)
    mn = -0.0 if normalize else -1.0
    assert float(torch.minimum(a.min(), b.min())) == mn and float(torch.maximum(a.max(), b.max())) == 1.0
    assert float(a.min()) > (0.0 if normalize else -1.0) and float(b.max()) < 1.0     # each extreme lives in one image only
    return lp_key(mn), lp_key(1.0)


def _s2d_pair(x1, x2):
    n, _, h, w = x1.shape
    bh, bw = stem_blocks(h, w)
    return torch.cat([lpips_ref.space_to_depth(TF.pad(x, (2, 2, 2, 2)), bh, bw) for x in (x1, x2)])


@functools.lru_cache(maxsize=None)
def prep_reference(normalize):
    """(ref, slack) float64 [2N,BH,BW,64]: the scaled, padded, space-to-depth tensor and 2^-22 (|x_in| + |shift_c|) / scale_c at
    the same places (zero in the padding ring and channels 48..63)."""
    a, b = prep_inputs(normalize)
    ref = _s2d_pair(lpips_ref.scale_input(a, normalize), lpips_ref.scale_input(b, normalize))
    sh = torch.tensor(lpips_ref.SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    sc = torch.tensor(lpips_ref.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    xin = lambda x: (2 * x.double() - 1 if normalize else x.double()).abs()
    slack = _s2d_pair((xin(a) + sh.abs()) / sc, (xin(b) + sh.abs()) / sc) * 2.0 ** -22
    return ref, slack


def prep_bound(normalize, dtype):
    """|got - ref64| <= 1/2 ulp16(ref) + 2^-22 (|x_in| + |shift_c|) / scale_c: one storage rounding plus the four fp32 roundings
    of (x - shift) / scale with fp32 constants (the two constants, the difference, the quotient; 2 raw - 1 is exact or rounds
    inside the same budget: |x_in| <= 1 and the bound carries |x_in| at full weight for each of the four)."""
    ref, slack = prep_reference(normalize)
    return 0.5 * ulp16(ref, dtype) + slack


def prep_fp32_emulation(normalize, dtype):
    """The kernel's arithmetic in torch fp32 on the CPU, rounded to the storage type."""
    a, b = prep_inputs(normalize)
    sh = torch.tensor(lpips_ref.SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    sc = torch.tensor(lpips_ref.SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    f = lambda x: ((2.0 * x - 1.0 if normalize else x) - sh) / sc
    return _s2d_pair(f(a), f(b)).to(dtype)


def prep_ring_mask():
    """True where the stem input has no image pixel: the 2-pixel padding ring, the rows / columns past the padded image, and
    channels 48..63."""
    n, h, w = PREP_SHAPE
    one = torch.ones(n, 3, h, w, dtype=torch.float64)
    return _s2d_pair(one, one) == 0


@functools.lru_cache(maxsize=None)
def prep_bwd_case(dtype, normalize):
    """(up [N,BH,BW,64] 16-bit, scale, float64 autograd of scale_input + pad + space_to_depth for up / scale)."""
    n, h, w = PREP_SHAPE
    bh, bw = stem_blocks(h, w)
    g = torch.Generator().manual_seed(1100 + int(normalize))
    up = torch.randn(n, bh, bw, 64, generator=g).to(dtype)
    scale = 1024.0
    x = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64).requires_grad_()
    lpips_ref.space_to_depth(TF.pad(lpips_ref.scale_input(x, normalize), (2, 2, 2, 2)), bh, bw).backward(up.double() / scale)
    return up, scale, x.grad


@functools.lru_cache(maxsize=None)
def pool_fwd_case():
    """(x [N,H,W,Cp] on the k/32 grid, |k| <= 255 -- exact in both 16-bit types --, max_pool2d of it in float64 NHWC).
    Planted: a NaN, a +Inf and a -Inf in three separate windows, and a NaN in the last window of the last image."""
    n, h, w, cp = POOL_SHAPE
    g = torch.Generator().manual_seed(1200)
    x = torch.randint(-255, 256, (n, h, w, cp), generator=g).double() / 32
    x[0, 10, 10, 3] = float("nan")
    x[0, 100, 200, 9] = float("inf")
    x[1, 301, 7, 63] = float("-inf")
    x[n - 1, h - 1, w - 1, 17] = float("nan")
    y = TF.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous()
    return x.float(), y.float()                          # (exact: kept in fp32 to hold a quarter GB less)


@functools.lru_cache(maxsize=None)
def pool_bwd_case():
    """(x on the k/8 grid with ties, dy and addend on the k/32 grid, float64 autograd of max_pool2d), all NHWC -- the gather form
    of test_host_lpips_grad.py takes 18 s at this shape and is pinned equal to autograd under ties there."""
    from test_host_lpips_grad import quantised
    n, h, w, cp = POOL_SHAPE
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    g = torch.Generator().manual_seed(1300)
    x = quantised((n, cp, h, w), 2, g)
    dy = torch.randint(-64, 65, (n, cp, oh, ow), generator=g).double() / 32
    add = torch.randint(-64, 65, (n, cp, h, w), generator=g).double() / 32
    xa = x.clone().requires_grad_()
    TF.max_pool2d(xa, 3, 2).backward(dy)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float()
    grad = nhwc(xa.grad)
    assert torch.equal(grad.double(), xa.grad.permute(0, 2, 3, 1))           # sums of at most four k/32: exact in fp32
    return nhwc(x), nhwc(dy), nhwc(add), grad            # NHWC fp32 (exact; a quarter GB less to hold than float64)


# ============================================================================= 2. LPIPS distance / finalize / distance-bwd
# name -> (N, [(hw, C, Cp), ...], feature scale per dtype or None).  hw = 129 * 128 = 16,512 pixels are 65 blocks per image:
# the k += 64 loop of lpips_finalize_kernel wraps.  N = 17 / 33 wrap its n += 16 loop once / twice.
DIST_CASES = {
    "hw-edges-5taps": (1, [(1, 64, 64), (31, 64, 64), (256, 64, 64), (257, 64, 64), (16512, 64, 64)], None),
    "wrap65-cp8": (2, [(16512, 8, 8)], None),
    "c3-of-8-1tap": (1, [(257, 3, 8)], None),
    "padded-2taps": (2, [(31, 60, 64), (256, 380, 384)], None),
    "alex-5taps": (3, [(257, 64, 64), (31, 192, 192), (1, 384, 384), (1, 256, 256), (1, 256, 256)], None),
    "n17-2taps": (17, [(1, 8, 8), (31, 3, 8)], None),
    "n33-1tap": (33, [(1, 64, 64)], None),
    "tiny-2taps": (2, [(31, 3, 8), (257, 64, 64)], {torch.float16: 1e-4, torch.bfloat16: 2e-5}),
}
DIST_TOTAL0, DIST_TOTAL_SCALE = 0.625, 0.375              # the running total and a total_scale that is not 1 / N
DIST_UP = (0.7, 0.05, 1.9)                                # upstream gradient per image, cycled (as test_gpu_lpips_grad.py)


def distance_blocks(taps, n):
    """(blocks per image of every tap, block count of the launch): lpips_table."""
    per = [-(-hw // LPIPS_PIX_PER_BLOCK) for hw, _, _ in taps]
    return per, n * sum(per)


@functools.lru_cache(maxsize=None)
def distance_inputs(name, dtype):
    """[(f [2N,hw,Cp] 16-bit, w [C] fp32)] per tap.  ReLU-like features, a quarter of the pixels dead in image 1 and another
    quarter in image 2 (one of the two shared), pad channels zero; in the tiny regime |f| ~ 1e-4 (fp16; 2e-5 in bf16), where
    the 1e-8 under the root is a visible share of sum f^2.
    With C <= 8 the first two channels are positive in every live pixel.  Left to the ReLU alone, one pixel in twenty of a C = 3
    tap has the same single live channel in both images: there n1 = n2 = 1 up to 1e-9, fp32 gives n1 - n2 = 0 or one ulp, and
    no fp32 evaluation of the backward can meet a bound that is relative to the true |n1 - n2| (the rule of
    test_gpu_lpips_grad.py, written for C >= 64, where two parallel feature vectors do not occur)."""
    n, taps, tiny = DIST_CASES[name]
    g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
    out = []
    for hw, c, cp in taps:
        f = torch.zeros(2 * n, hw, cp)
        f[..., :c] = TF.relu(torch.randn(2 * n, hw, c, generator=g))
        if c <= 8:
            f[..., :2] = torch.randn(2 * n, hw, 2, generator=g).abs() + 0.05
        if tiny:
            f = f * tiny[dtype]
        pn = torch.arange(hw).view(1, hw) + torch.arange(n).view(n, 1)
        f[:n][(pn % 4) == 1] = 0
        f[n:][((pn % 8) == 1) | ((pn % 8) == 2)] = 0
        out.append((f.to(dtype), torch.rand(c, generator=g) + 0.05))
    return out


def _norms(f64, c, eps_mode="root"):
    s = (f64[..., :c] ** 2).sum(-1, keepdim=True)
    if eps_mode == "root":
        return f64[..., :c] / torch.sqrt(1e-8 + s)
    if eps_mode == "norm":
        return f64[..., :c] / (torch.sqrt(s) + 1e-8)
    return torch.where(s > 0, f64[..., :c] / torch.sqrt(s.clamp_min(1e-300)), torch.zeros_like(f64[..., :c]))    # eps omitted


def distance_reference(name, dtype, mutant=None, fp=torch.float64):
    """[N] per-image distance: sum_t (1 / hw_t) sum_p sum_{c < C} w[c] (n1 - n2)^2 in `fp`, or one of the wrong variants the
    tolerance has to reject (tests/test_host_loss_sweep.py)."""
    n, taps, _ = DIST_CASES[name]
    out = torch.zeros(n, dtype=fp)
    for (hw, c, cp), (f, w) in zip(taps, distance_inputs(name, dtype)):
        f, w = f.to(fp), w.to(fp)
        f1, f2 = f[:n], f[n:]
        if mutant == "pair-next-image":
            f2 = torch.roll(f2, -1, 0)
        if mutant == "channel-C-included" and c < cp:
            # one channel more, weighted by the float that follows the C weights in memory: the (NaN) sentinel margin
            c, w = c + 1, torch.cat([w, torch.full((1,), float("nan"), dtype=fp)])
        if mutant == "weights-shifted":
            w = torch.roll(w, -1)
        mode = {"eps-on-norm": "norm", "eps-omitted": "none"}.get(mutant, "root")
        d = _norms(f1, c, mode) - _norms(f2, c, mode)
        per_pix = (d * d * w).sum(-1)
        if mutant == "last-pixel-dropped":
            per_pix = per_pix[:, :-1]
        out = out + per_pix.sum(-1) / (taps[0][0] if mutant == "hw-of-tap-0" else hw)
    return out


DIST_MUTANTS = ("eps-on-norm", "eps-omitted", "hw-of-tap-0", "last-pixel-dropped", "weights-shifted", "channel-C-included",
                "pair-next-image")


def distance_tolerance(name, dtype):
    """[N] allowed |got - ref64| of a per-image distance, u = 2^-24, first order in u plus the e^2 term:
      * sum f^2 over C channels: C product roundings and at most C - 1 inexact adds in any chain (a lane adds zeros for the pad
        channels and the vectors it does not own: exact), + the eps add: (C + 1) u relative; the root halves it and adds u, the
        reciprocal and the product with f add u each: (C / 2 + 3.5) u <= (C / 2 + 5) u relative on n1 and n2;
      * d = n1 - n2: e = (C / 2 + 5) u (|n1| + |n2|) + u |d| absolute;
      * w d^2: w (2 |d| e + e^2) + 2 u w d^2 (d * d and the product with w round once each, contraction is off);
      * the sum of these non-negative terms: depth u relative, depth = 384 sequential adds of a thread (8 pixels x 48 channels)
        + 6 (wave tree) + 2 (the four waves) + ceil(nblk / 64) + 6 (finalize: a lane's partials, its wave tree) + 1 (the
        division by hw) + 5 (the sum over taps)."""
    n, taps, _ = DIST_CASES[name]
    tol = torch.zeros(n, dtype=torch.float64)
    ref = torch.zeros(n, dtype=torch.float64)
    depth = 0
    for (hw, c, cp), (f, w) in zip(taps, distance_inputs(name, dtype)):
        f, w = f.double(), w.double()
        n1, n2 = _norms(f[:n], c), _norms(f[n:], c)
        d = (n1 - n2).abs()
        e = (c / 2 + 5) * U32 * (n1.abs() + n2.abs()) + U32 * d
        tol += (w * (2 * d * e + e * e) + 2 * U32 * w * d * d).sum((-1, -2)) / hw
        ref += (w * d * d).sum((-1, -2)) / hw
        nblk = -(-hw // LPIPS_PIX_PER_BLOCK)
        depth = max(depth, 384 + 6 + 2 + -(-nblk // 64) + 6 + 1 + 5)
    return tol + depth * U32 * ref


def distance_total(per64, n, accumulate):
    """float64 total: total_scale * sum_n per_image[n], on top of the running total with `accumulate`."""
    scale = DIST_TOTAL_SCALE if accumulate else 1.0 / n
    return (DIST_TOTAL0 if accumulate else 0.0) + scale * float(per64.sum())


def distance_total_tolerance(per64, tol, n, accumulate):
    """The per-image allowances, + (ceil(N / 16) + 16 + 2) u relative on the scaled sum (a wave's images, the 16 wave sums, the
    fp32 total_scale and its product), + one rounding of the accumulated total."""
    scale = DIST_TOTAL_SCALE if accumulate else 1.0 / n
    t = scale * float(tol.sum()) + (-(-n // 16) + 18) * U32 * scale * float(per64.sum())
    return t + (U32 * abs(distance_total(per64, n, True)) if accumulate else 0.0)


EPS16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}                # half an ulp, relative: one rounding to storage


def distance_bwd_scale(name):
    """Loss scale of the backward cases: 256, and 2^-4 in the tiny regime, where 1 / s reaches 1e4 and fp16 would saturate."""
    return 2.0 ** -4 if DIST_CASES[name][2] else 256.0


def distance_upstream(n):
    return torch.tensor([DIST_UP[i % 3] for i in range(n)], dtype=torch.float32)


def distance_bwd_reference(name, dtype):
    """Per tap (ref, tol), float64 [2N,hw,C]: the image-1 half then the image-2 half of dsr_lpips_distance_bwd (ReLU mask and
    loss scale included) and the per-element rule of test_gpu_lpips_grad.py::test_distance_bwd_vs_float64: two storage roundings
    relative to |ref|, + C 2^-24 relative to the absolute sums the two channel reductions accumulate (|f|^2 under the root,
    <|u|, |n|> in the projection), + half an fp16 subnormal step in fp16."""
    from test_host_lpips_grad import distance_grads
    n, taps, _ = DIST_CASES[name]
    g = distance_upstream(n).double() * distance_bwd_scale(name)
    out = []
    for (hw, c, cp), (f, w) in zip(taps, distance_inputs(name, dtype)):
        f = f.double()[..., :c].permute(0, 2, 1).unsqueeze(-1)               # [2N,C,hw,1]
        f1, f2 = f[:n], f[n:]
        r1, r2 = distance_grads(f1, f2, w, g)
        refs, tols = [], []
        for ref, fa, fb in ((r1 * (f1 > 0), f1, f2), (r2 * (f2 > 0), f2, f1)):
            sa = torch.sqrt(1e-8 + (fa * fa).sum(1, keepdim=True))
            sb = torch.sqrt(1e-8 + (fb * fb).sum(1, keepdim=True))
            na, nb = fa / sa, fb / sb
            u = (2 * w.double().view(1, -1, 1, 1) * (na - nb) * g.view(-1, 1, 1, 1) / hw).abs()
            acc = c * U32 * (4 * u + 4 * na * (u * na).sum(1, keepdim=True)) / sa
            refs.append(ref)
            tols.append(2 * EPS16[dtype] * ref.abs() + acc + (2.0 ** -25 if dtype == torch.float16 else 0.0))
        back = lambda ts: torch.cat(ts).squeeze(-1).permute(0, 2, 1).contiguous()
        out.append((back(refs), back(tols)))
    return out


def distance_bwd_fp32(name, dtype):
    """The kernel's formulas in torch fp32 on the CPU, stored in the 16-bit type (fp16 saturating): per tap [2N,hw,C]."""
    n, taps, _ = DIST_CASES[name]
    g = distance_upstream(n) * distance_bwd_scale(name)
    out = []
    for (hw, c, cp), (f, w) in zip(taps, distance_inputs(name, dtype)):
        f = f.float()[..., :c]
        x1, x2 = f[:n], f[n:]
        r1 = 1.0 / torch.sqrt(1e-8 + (x1 * x1).sum(-1, keepdim=True))
        r2 = 1.0 / torch.sqrt(1e-8 + (x2 * x2).sum(-1, keepdim=True))
        n1, n2 = x1 * r1, x2 * r2
        u = w * (n1 - n2) * (2.0 * (g / hw)).view(-1, 1, 1)
        d1 = torch.where(x1 > 0, (u - n1 * (u * n1).sum(-1, keepdim=True)) * r1, torch.zeros(()))
        d2 = torch.where(x2 > 0, (n2 * (u * n2).sum(-1, keepdim=True) - u) * r2, torch.zeros(()))
        d = torch.cat([d1, d2])
        out.append((d.clamp(-65504.0, 65504.0) if dtype == torch.float16 else d).to(dtype))
    return out


# ============================================================================= 3. feature-loss taps
FEAT_P = 70001
FEAT_FWD = (FEAT_P, 8, 5)             # P, Cp, C
FEAT_BWD = (FEAT_P, 64, 64)
FEAT_COEF = 2.0 ** -4


def reduce_blocks(p, target=1024):
    """(blocks, rows per block) of dsr_pw_reduce_blocks at its default target."""
    rpb = max(64, -(-p // target))
    return -(-p // rpb), rpb


def int_maps(p, cp, c, dtype, seed):
    """f, t in [-4, 4], dnext in [-3, 3], integers, pad channels zero (the maps of test_gpu_vggfeat.py::_int_maps as [P, Cp])."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randint(-4, 5, (p, cp), generator=g).float()
    t = torch.randint(-4, 5, (p, cp), generator=g).float()
    dn = torch.randint(-3, 4, (p, cp), generator=g).float()
    for m in (f, t, dn):
        m[:, c:] = 0
    return f.to(dtype), t.to(dtype), dn.to(dtype)


def feat_partials(f, t, mode, rpb):
    """Exact per-block sums [blocks] (float64 integers) of |f - t| or (f - t)^2 over the block's rows."""
    d = f.double() - t.double()
    rows = (d.abs() if mode == 0 else d * d).sum(1)
    blocks = -(-rows.numel() // rpb)
    pad = torch.zeros(blocks * rpb, dtype=torch.float64)
    pad[:rows.numel()] = rows
    return pad.view(blocks, rpb).sum(1)


# ============================================================================= 4. pixel-loss glue
DIFF_SIZES = (1, 255, 3 * 1024 + 5, 2 ** 20 + 7)
AXPBY_SIZES = (1, 257, 2 ** 20 + 3)
BCE_SIZES = (1, 256, 257, 1000)


def gan_loss_blocks(n):
    return min(1024, -(-n // 1024))


def diff_inputs(n):
    """pred, tgt fp32 on the k/8 grid, |k| <= 8: every difference, square, per-thread sum and block partial is exact in fp32."""
    g = torch.Generator().manual_seed(4000 + n % 1000)
    pred = torch.randint(-8, 9, (n,), generator=g).float() / 8
    tgt = torch.randint(-8, 9, (n,), generator=g).float() / 8
    return pred, tgt


def diff_partials(pred, tgt, mode, blocks):
    """[blocks] float64: block b owns the elements i with (i // 256) % blocks == b (diff_loss_kernel's grid-stride loop)."""
    d = pred.double() - tgt.double()
    e = d.abs() if mode == 0 else d * d
    owner = (torch.arange(e.numel()) // 256) % blocks
    return torch.zeros(blocks, dtype=torch.float64).index_add_(0, owner, e)


def diff_grad32(pred, tgt, mode):
    """The kernel's fp32 expression: sign(d) * fl(1 / n), or fl(fl(2 d) * fl(1 / n)) (2 d is exact)."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(pred.numel()), dtype=torch.float32)
    d = pred - tgt
    return torch.sign(d) * inv if mode == 0 else (2.0 * d) * inv


def torch_nonfinite_diff(mode):
    """(pred, tgt, loss, grad) of torch's l1_loss / mse_loss (fp32, CPU) on a vector with a NaN, a +Inf and a -Inf difference."""
    pred = torch.tensor([0.5, float("nan"), float("inf"), float("-inf"), -0.25, 0.0, 1.0, 0.125], requires_grad=True)
    tgt = torch.tensor([0.25, 0.0, 0.0, 0.0, -0.25, 0.5, 1.0, 0.0])
    loss = (TF.l1_loss if mode == 0 else TF.mse_loss)(pred, tgt)
    (grad,) = torch.autograd.grad(loss, pred)
    return pred.detach(), tgt, loss.detach(), grad


AXPBY_A, AXPBY_B, AXPBY_G = 1.5, -0.25, 0.3


def axpby_inputs(n):
    """x, y on the k/8 grid (|k| <= 32) with a = 1.5, b = -0.25: a x, b y and their sum are exact in fp32, so a fused and an
    unfused a x + b y give the same bits; the product with g = fl(0.3) rounds once."""
    g = torch.Generator().manual_seed(4100 + n % 1000)
    return (torch.randint(-32, 33, (n,), generator=g).float() / 8, torch.randint(-32, 33, (n,), generator=g).float() / 8)


def axpby_expected(x, y, with_y, with_g):
    s = AXPBY_A * x.double() + (AXPBY_B * y.double() if with_y else 0.0)
    assert torch.equal(s.float().double(), s)
    gs = torch.tensor(AXPBY_G, dtype=torch.float32) if with_g else torch.tensor(1.0)
    return s.float() * gs


def bce_inputs(n):
    """Probabilities in (0, 1) with p = 0 and p = 1 planted (the -100 clamp of the logarithm); one value: p = 0."""
    g = torch.Generator().manual_seed(4200 + n)
    p = torch.rand(n, generator=g).clamp(1e-6, 1 - 1e-6)
    p[0] = 0.0
    if n > 1:
        p[n - 1] = 1.0
    return p


def bce_reference(p, target, fp):
    """(mean BCE, its gradient) of torch.nn.functional.binary_cross_entropy in `fp` against the constant target."""
    x = p.to(fp).requires_grad_()
    loss = TF.binary_cross_entropy(x, torch.full_like(x, target))
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), grad


def is_past(items, cap):
    """More than one grid pass, and the second one ragged (not every thread of the grid has a second item)."""
    return cap < items < 2 * cap
