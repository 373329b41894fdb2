"""Case tables, float64 / exact references, derived bounds and the restated launcher arithmetic of the style-kernel sweep
(tests/test_host_style_sweep.py on the CPU, tests/test_gpu_style_sweep.py on the device): csrc/featstyle.hip -- dsr_gram_fwd,
dsr_gram_loss and dsr_featstyle_tap_bwd -- at the shapes where each kernel leaves its first regime.  Test infrastructure: the
package never imports it.

Every threshold below restates a launcher's own arithmetic next to the constant it uses; the host test asserts each case
against these AND against what the ABI reports (dsr_gram_chunks, dsr_gram_workspace), and asserts that every branch a
production tap takes is taken by a case, so a changed cap turns a case red instead of moving it back into the first regime.

The `variant=` arguments of the emulations are the wrong kernels the cases are there to catch; the host test shows, on the
CPU, which case rejects each of them."""
import collections
import functools
import math
from fractions import Fraction

import numpy as np
import torch

MARGIN = 1024          # sentinel elements on each side of a raw buffer: 2 KB, 4 KB or 8 KB, always a multiple of 16 bytes
SENTINEL = -7777.25    # no integer and no integer / 64: no exact case produces it
NAN = float("nan")

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # unit roundoff of the 16-bit formats
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}  # half the spacing of their subnormals

# ---------------------------------------------------------------- the launchers' arithmetic (csrc/featstyle.hip, include/dsr_hip.h)
GRAM_CHUNK = 1024                  # pixels per partial slab
GRAM_KP = 128                      # pixels staged per step of gram_fwd_kernel
GRAM_FOLD_CAP = 4096 * 256         # items of gram_fold_kernel's grid; it strides beyond
LOSS_SLICE_ENTRIES = 8192          # entries per block of gram_loss_reduce_kernel (style_loss_slices)
DSR_GRAM_LOSS_SLICES = 32
GRAM_LOSS_PARTIALS = 2 * DSR_GRAM_LOSS_SLICES      # doubles of scratch per image
LOSS_FOLD_THREADS = 256            # gram_loss_fold_kernel: one block, strided beyond
STYLE_MAX_CP = 512
TILE = 64                          # channel tile, K step and pixel tile of the two MFMA kernels


def chunks(hw):
    return -(-hw // GRAM_CHUNK)


def tiles(cp):
    return -(-cp // TILE)


def pairs(cp):
    return tiles(cp) * (tiles(cp) + 1) // 2


def fold_items(n, c):
    return n * c * c


def slices(c):
    return min(DSR_GRAM_LOSS_SLICES, max(1, -(-c * c // LOSS_SLICE_ENTRIES)))


def per(c):
    return -(-c * c // slices(c))


def loss_terms(n, c):
    return n * slices(c)


def ksteps(cp):
    return -(-cp // TILE)


def pixel_tiles(hw):
    return -(-hw // TILE)


Regime = collections.namedtuple("Regime", "tiles last_tile_partial pad multi_chunk last_chunk fold_past_cap "
                                          "slices last_slice_ragged terms_past_256 "
                                          "ksteps last_kstep_ragged last_pixel_tile_ragged")
# the components that concern each kernel (the backward's channel tiles are its K steps: both are ceil(Cp / 64))
REGIME_FIELDS = {"fwd": ("tiles", "last_tile_partial", "pad", "multi_chunk", "last_chunk", "fold_past_cap"),
                 "loss": ("pad", "slices", "last_slice_ragged", "terms_past_256"),
                 "bwd": ("pad", "ksteps", "last_kstep_ragged", "last_pixel_tile_ragged")}


def regime(n, hw, c, cp):
    """The branches a shape takes.  last_chunk classes the pixels of an image's last chunk by what the staging loop does with
    them: "one" (a single pixel), "ragged" (not a multiple of GRAM_KP: the `in` guard zero-fills inside the last step) or "full"
    (whole steps only, 1024 pixels or fewer: the guard never cuts)."""
    last = hw - (chunks(hw) - 1) * GRAM_CHUNK
    return Regime(tiles=tiles(cp), last_tile_partial=cp % TILE != 0, pad=c < cp, multi_chunk=chunks(hw) > 1,
                  last_chunk="one" if last == 1 else ("ragged" if last % GRAM_KP else "full"),
                  fold_past_cap=fold_items(n, c) > GRAM_FOLD_CAP,
                  slices=slices(c), last_slice_ragged=per(c) * slices(c) != c * c,
                  terms_past_256=loss_terms(n, c) > LOSS_FOLD_THREADS,
                  ksteps=ksteps(cp), last_kstep_ragged=cp % TILE != 0, last_pixel_tile_ragged=hw % TILE != 0)


# ---------------------------------------------------------------- raw buffers
def bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guard:
    """Buffers between MARGIN sentinel elements on each side (a multiple of 16 bytes for every type: the entry points'
    alignment checks still pass).  new(): an output, pre-filled with the sentinel.  put(): an input between NaN margins, so that
    a read past either end that stays inside the allocation poisons the result.  check(): every margin kept its bits."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, shape, dtype, fill=SENTINEL, margin=SENTINEL):
        numel = math.prod(shape)
        flat = torch.full((numel + 2 * MARGIN,), margin, dtype=dtype, device=self.dev)
        flat[MARGIN:MARGIN + numel] = fill
        self.bufs.append((flat, bits(flat[:MARGIN]).clone(), bits(flat[-MARGIN:]).clone()))
        return flat[MARGIN:MARGIN + numel].view(shape)

    def put(self, t, margin=NAN):
        v = self.new(tuple(t.shape), t.dtype, margin=margin)
        v.copy_(t)
        return v

    def check(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        for flat, lo, hi in self.bufs:
            assert torch.equal(bits(flat[:MARGIN]), lo) and torch.equal(bits(flat[-MARGIN:]), hi), "write outside a tensor"


def f32_of(fr):
    """Fraction -> double is correctly rounded; the kernel rounds the same double quotient to fp32."""
    return np.float32(float(fr))


# ============================================================================= 1. Gram forward
# name -> (N, HW, C, Cp); integers in [-3, 3], pad channels zero: every sum is at most 9 HW < 2^24, exact in fp32 in any order
FWD_CASES = {
    "cp72": (2, 200, 72, 72),              # two tiles, the second 8 channels wide; ragged second staging step
    "cp200-pad": (1, 130, 197, 200),       # four tiles, ten pairs, pad channels; gram's row stride odd
    "cp512-edge": (1, 1025, 512, 512),     # 36 pairs; two chunks, the second one pixel
    "hw1024": (2, 1024, 64, 64),           # one chunk, exactly full
    "hw2048": (2, 2048, 64, 64),           # two chunks, exactly full
    "chunks9": (3, 8193, 5, 8),            # nine chunks in each of three images, the last one pixel
    "foldcap": (5, 7, 459, 464),           # 1 053 405 fold items > 1 048 576; last tile 16 channels; pad channels
}
FWD_SCALES = (1.0, 2.0 ** -6)


def int_map(shape, c, lo, hi, seed):
    """fp32 integers in [lo, hi], channels >= c zero: exact in both 16-bit types."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, hi + 1, shape, generator=g).float()
    x[..., c:] = 0
    return x


@functools.lru_cache(maxsize=None)
def fwd_input(name):
    """[N, HW, Cp] fp32 integers; the last pixel of every image is non-zero in channel 0, so a one-pixel last chunk counts."""
    n, hw, c, cp = FWD_CASES[name]
    assert 9 * hw < 2 ** 24
    x = int_map((n, hw, cp), c, -3, 3, 500 + sum(map(ord, name)))
    x[:, -1, 0] = 3
    return x


def chunk_products(x, fp=torch.float64):
    """[N, chunks, Cp, Cp]: F^T F over each chunk of GRAM_CHUNK pixels, accumulated in `fp` (what a slab holds on and above
    the diagonal)."""
    n, hw, cp = x.shape
    k = chunks(hw)
    pad = torch.zeros(n, k * GRAM_CHUNK, cp, dtype=fp)
    pad[:, :hw] = x.to(fp)
    pad = pad.view(n * k, GRAM_CHUNK, cp)
    return (pad.transpose(1, 2) @ pad).view(n, k, cp, cp)


def fold_slabs(slabs, c, scale, fp=torch.float64, variant=None, fill=SENTINEL):
    """gram_fold_kernel on [N, chunks, Cp, Cp] slabs: the slabs summed in chunk order in `fp`, times scale, written as
    [N, C, C] over a buffer that held `fill`.
    variant "one-grid-pass": the stride loop's second pass is missing; "chunks-1": the last slab is left out;
    "row-stride-cp": entry (i, j) of image n is written at n C C + i Cp + j (in index order, inside the buffer)."""
    n, k, cp, _ = slabs.shape
    s = torch.zeros(n, cp, cp, dtype=fp)
    for q in range(k - 1 if variant == "chunks-1" else k):
        s = s + slabs[:, q].to(fp)
    g = (s[:, :c, :c] * torch.tensor(scale, dtype=fp)).contiguous()
    if variant == "one-grid-pass":
        flat = g.reshape(-1).clone()
        flat[GRAM_FOLD_CAP:] = fill
        g = flat.view(n, c, c)
    if variant == "row-stride-cp":
        flat = torch.full((n * c * c,), fill, dtype=fp)
        idx = (torch.arange(n).view(n, 1, 1) * c * c + torch.arange(c).view(1, c, 1) * cp + torch.arange(c).view(1, 1, c)).reshape(-1)
        ok = idx < flat.numel()
        flat[idx[ok]] = g.reshape(-1)[ok]
        g = flat.view(n, c, c)
    return g


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
    """(slabs [N, chunks, Cp, Cp], gram [N, C, C] at scale 1), float64 and exact."""
    c = FWD_CASES[name][2]
    slabs = chunk_products(fwd_input(name))
    return slabs, fold_slabs(slabs, c, 1.0)


FWD_VARIANTS = ("one-grid-pass", "chunks-1", "row-stride-cp")


# ============================================================================= 2. Gram loss
# (N, C, Cp): integer matrices in [-20, 20]
LOSS_CASES = {
    "c90-1slice": (3, 90, 96),
    "c91-2slices-ragged": (3, 91, 96),
    "c128-2slices": (3, 128, 128),
    "c200-5slices": (2, 200, 200),
    "c256-8slices": (2, 256, 256),
    "c512-32slices": (2, 512, 512),
    "n129-258terms": (129, 91, 96),         # grid.y = 129
    "n9-288terms": (9, 512, 512),
}
PLANT = 37


def _loss_matrices(n, c, seed):
    """G, Gt in [-18, 18] (every difference within 36), then: the last entry of image 0 (the last element of its last slice) and
    the first entry of the last image (the first element of its slice 0) differ by PLANT = 37, each the largest magnitude of
    its image, with G and Gt still in [-20, 20]; image 1, where there are three images or more, has G == Gt.  (With N = 2 the
    two planted images are all there is: the G == Gt image is checked in the cases with N >= 3, at 1, 2 and 32 slices.)"""
    g = torch.Generator().manual_seed(seed)
    gf = torch.randint(-18, 19, (n, c, c), generator=g)
    gt = torch.randint(-18, 19, (n, c, c), generator=g)
    gf[0, c - 1, c - 1], gt[0, c - 1, c - 1] = 20, 20 - PLANT
    gf[n - 1, 0, 0], gt[n - 1, 0, 0] = 20 - PLANT, 20
    if n >= 3:
        gt[1] = gf[1]
    return gf, gt


@functools.lru_cache(maxsize=None)
def loss_input(name):
    n, c, _ = LOSS_CASES[name]
    return _loss_matrices(n, c, 700 + c + n)


def loss_partials(d, mode):
    """Exact per-slice (sums, maxima) [N, slices] int64 of |d| or d^2 and of |d| over gram_loss_reduce_kernel's split."""
    n, c, _ = d.shape
    s, p = slices(c), per(c)
    flat = torch.zeros(n, s * p, dtype=torch.int64)
    flat[:, :c * c] = d.reshape(n, -1)
    flat = flat.view(n, s, p)
    return (flat.abs() if mode == 0 else flat * flat).sum(2), flat.abs().amax(2)


def loss_expected(d, mode, variant=None):
    """(value fp32, s_scale [N] fp32) of dsr_gram_loss on the integer difference d [N, C, C].
    variant "no-last-slice": gram_loss_reduce_kernel skips b == slices - 1 (its partial stays 0); "max-slice-0": the operand
    kernel takes the maximum from slice 0 alone; "terms-256": gram_loss_fold_kernel stops after its first 256 terms."""
    n, c, _ = d.shape
    sums, maxs = loss_partials(d, mode)
    if variant == "no-last-slice":
        sums, maxs = sums.clone(), maxs.clone()
        sums[:, -1], maxs[:, -1] = 0, 0
    total = int(sums.reshape(-1)[:LOSS_FOLD_THREADS].sum()) if variant == "terms-256" else int(sums.sum())
    mx = (maxs[:, 0] if variant == "max-slice-0" else maxs.amax(1)).float()
    scale = torch.ones(n) if mode == 0 else torch.where(mx > 0, mx, torch.ones(n))
    return f32_of(Fraction(total, n * c * c)), scale


LOSS_VARIANTS = ("no-last-slice", "max-slice-0", "terms-256")

NONFINITE_SHAPE = (3, 256, 256)          # N, C, Cp of the Gram matrices; the backward runs on a (3, 64, 256, 256) map
NONFINITE_AT = (1, 255, 250)             # image 1, an entry of its last slice
NONFINITE_HW = 64


@functools.lru_cache(maxsize=None)
def nonfinite_input():
    n, c, _ = NONFINITE_SHAPE
    assert (NONFINITE_AT[1] * c + NONFINITE_AT[2]) // per(c) == slices(c) - 1 == 7
    gf, gt = _loss_matrices(n, c, 900)
    gt[1] = gf[1] - (torch.arange(c * c).view(c, c) % 7 - 3)              # image 1 is an ordinary image here: |d| <= 3
    f = int_map((n, NONFINITE_HW, c), c, -3, 3, 901)
    f[f == 0] = 1                                                         # no zero: Inf * f is an Inf, never a NaN by accident
    return gf, gt, f


def torch_nonfinite_gram(mode, bad):
    """torch in float64 on the non-finite case: (value, dG [N, C, C], F . dG [N, HW, C]) of mean |G - Gt| or mean (G - Gt)^2
    with `bad` at NONFINITE_AT of G; F . dG is what the backward GEMM makes of that gradient."""
    import torch.nn.functional as TF
    gf, gt, f = nonfinite_input()
    g = gf.double()
    g[NONFINITE_AT] = bad
    g.requires_grad_()
    value = (TF.l1_loss if mode == 0 else TF.mse_loss)(g, gt.double())
    (dg,) = torch.autograd.grad(value, g)
    return value.detach(), dg, f.double() @ dg


# ============================================================================= 3. tap backward
BWD_CASES = {
    "hw64": (3, 64, 64, 64),
    "cp72": (2, 65, 72, 72),
    "cp200-pad": (1, 130, 197, 200),
    "cp512": (2, 70, 512, 512),
}
BWD_ALL_FLAGS = ("cp72", "cp512")        # every combination of masked, dnext, content and mode; the others: all on, style only
# power-of-two scalars: the content term's 2^-9 under style sums of several units spans more than 11 bits, so the one rounding
# does round, in both formats
G_STYLE, COEF_STYLE, G_CONTENT, COEF_CONTENT = 0.5, 2.0 ** -3, 2.0, 2.0 ** -10


def bwd_flags(name):
    """(mode, masked, with_next, with_content) of every run of a case; the mode only enters through the content term."""
    if name in BWD_ALL_FLAGS:
        return [(mode, m, nx, ct) for mode in (0, 1) for m in (0, 1) for nx in (False, True) for ct in (False, True)
                if mode == 0 or ct]
    return [(0, 1, True, True), (1, 1, True, True), (0, 0, False, False)]


@functools.lru_cache(maxsize=None)
def bwd_input(name):
    """f, t, dnext [N, HW, Cp] integers in [-3, 3] with zero pad channels, a NON-symmetric integer s16 [N, Cp, Cp] in [-2, 2]
    with zero pad rows and columns, s_scale[n] = 2^(n - 1): all fp32, exact in both 16-bit types."""
    n, hw, c, cp = BWD_CASES[name]
    assert 6 * cp <= 3072
    seed = 800 + sum(map(ord, name))
    f, t, dn = (int_map((n, hw, cp), c, -3, 3, seed + k) for k in range(3))
    s = int_map((n, cp, cp), c, -2, 2, seed + 3)
    s[:, c:, :] = 0
    assert not torch.equal(s, s.transpose(1, 2))
    return f, t, dn, s, torch.tensor([2.0 ** (k - 1) for k in range(n)])


def bwd_expected(name, mode, masked, with_next, with_content, variant=None):
    """float64 df [N, HW, Cp] of dsr_featstyle_tap_bwd on the integer case, exact in fp32 (asserted).
    variant "k448": the GEMM's K loop stops at channel 448; "s16-transposed": s16[n][c][i] in place of s16[n][i][c]."""
    f, t, dn, s, ss = (v.double() for v in bwd_input(name))
    k = 448 if variant == "k448" else f.shape[2]
    sm = s.transpose(1, 2) if variant == "s16-transposed" else s
    gemm = f[..., :k] @ sm[:, :k]
    assert float(gemm.abs().max()) <= 6 * f.shape[2]
    want = G_STYLE * COEF_STYLE * ss[:, None, None] * gemm
    if with_next:
        want = want + (dn * (f > 0).double() if masked else dn)
    if with_content:
        x = f - t
        want = want + G_CONTENT * COEF_CONTENT * (torch.sign(x) if mode == 0 else 2.0 * x)
    assert torch.equal(want.float().double(), want)
    return want


BWD_VARIANTS = ("k448", "s16-transposed")


# ============================================================================= 4. float data against float64
FLOAT_CASES = {"2x1030x512": (2, 1030, 512, 512), "1x200x72": (1, 200, 72, 72)}


@functools.lru_cache(maxsize=None)
def float_input(name, dtype):
    """f, t [N, HW, Cp]: N(0, 1) rounded to 16 bits, pad channels zero."""
    n, hw, c, cp = FLOAT_CASES[name]
    g = torch.Generator().manual_seed(31 + hw)
    f = torch.randn((n, hw, cp), generator=g)
    t = torch.randn((n, hw, cp), generator=g)
    f[..., c:] = 0
    t[..., c:] = 0
    return f.to(dtype), t.to(dtype)


def float_scale(name):
    n, hw, c, cp = FLOAT_CASES[name]
    return 1.0 / (c * hw)


@functools.lru_cache(maxsize=None)
def float_fwd_reference(name, dtype, which):
    """(G64, bound) [N, C, C] of map `which` (0: f, 1: t): the float64 Gram matrix of the 16-bit values and
    (HW + chunks + 2) 2^-24 scale |F|^T |F| (test_gpu_vggstyle.py::test_kernels_on_float_maps_against_float64)."""
    n, hw, c, cp = FLOAT_CASES[name]
    x = float_input(name, dtype)[which].double()
    scale = float_scale(name)
    ref = (x.transpose(1, 2) @ x)[:, :c, :c] * scale
    mag = (x.abs().transpose(1, 2) @ x.abs())[:, :c, :c] * scale
    return ref, (hw + chunks(hw) + 2) * 2.0 ** -24 * mag


def float_loss_reference(d64, mode):
    """float64 value of the loss on the kernel's own fp32 Gram matrices (D = G - Gt, exact in float64); its bound is 2^-23
    relative."""
    return float(d64.abs().mean() if mode == 0 else (d64 * d64).mean())


def float_bwd_reference(name, dtype, d64, mode):
    """(coef, g_up, R, bound): the style-only backward against R = k F D (D the difference of the kernel's own fp32 Gram
    matrices, sign(D) for L1), k = g_up coef, with
        |df - R| <= E + u (|R| + E) + tiny,    E = |k| (u [MSE only] + 2^-23 + (Cp + 4) 2^-24) (|F| |D|)
    as derived in test_gpu_vggstyle.py.  coef is the fp32 value FeatureStyleTap passes; g_up = 3 * 2^e plays the loss scale's
    part and puts the largest |R| in [3, 6)."""
    n, hw, c, cp = FLOAT_CASES[name]
    u = U[dtype]
    f64 = float_input(name, dtype)[0].double()
    coef = float(np.float32((2.0 if mode == 0 else 4.0) * float_scale(name) / (n * c * c)))
    dp = torch.zeros(n, cp, cp, dtype=torch.float64)
    dp[:, :c, :c] = torch.sign(d64) if mode == 0 else d64
    fd0 = f64 @ dp
    g_up = 3.0 * 2.0 ** -math.floor(math.log2(coef * float(fd0.abs().max())))
    k = g_up * coef
    r = k * fd0
    fd = abs(k) * (f64.abs() @ dp.abs())
    e = ((u if mode == 1 else 0.0) + 2.0 ** -23 + (cp + 4) * 2.0 ** -24) * fd
    return coef, g_up, r, e + u * (r.abs() + e) + TINY[dtype]


def emulate_loss_operand(d64, mode, dtype):
    """(value fp32, s16 [N, C, C] 16-bit, s_scale [N] fp32) as dsr_gram_loss forms them: double sums and one rounding for the
    value, the fp32 difference, its fp32 quotient by the largest magnitude and one rounding to 16 bits for the operand."""
    n = d64.shape[0]
    value = np.float32(float((d64.abs() if mode == 0 else d64 * d64).sum()) / d64.numel())
    d32 = d64.float()
    if mode == 0:
        return value, torch.sign(d32).to(dtype), torch.ones(n)
    mx = d32.abs().reshape(n, -1).amax(1)
    div = torch.where(mx > 0, mx, torch.ones(n))
    return value, (d32 / div[:, None, None]).to(dtype), div


def emulate_bwd_style_only(f16, s16, s_scale, g_up, coef, c):
    """The style-only backward in fp32 on the CPU: fp32 GEMM of f with the 16-bit operand, the three fp32 products of the
    epilogue, one rounding to the map's type."""
    n, hw, cp = f16.shape
    sp = torch.zeros(n, cp, cp)
    sp[:, :c, :c] = s16.float()
    ks = (torch.tensor(g_up, dtype=torch.float32) * torch.tensor(coef, dtype=torch.float32)) * s_scale.float()
    return (ks[:, None, None] * (f16.float() @ sp)).to(f16.dtype)


def worst_ratio(err, bound):
    """Largest err / bound; where nothing is allowed (bound == 0) there must be no error."""
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "a deviation where the allowance is zero"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


CACHES = (fwd_input, fwd_reference, loss_input, nonfinite_input, bwd_input, float_input, float_fwd_reference)


def drop_caches():
    for f in CACHES:
        f.cache_clear()
