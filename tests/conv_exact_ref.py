"""Exact-integer reference of one convolution layer, forward and backward, in float64 on the CPU.

Small-integer operands make every product and every partial sum of a convolution exact in fp32 (below 2^24), so a kernel's
result no longer depends on summation order, MFMA shape or split-K: the only rounding left is the final store to 16 bits,
and that one is defined (round to nearest even).  This module restates the layer as plain sums over taps -- no unfold through
the kernels' own decompositions, nothing imported from the package under test but its constants -- and holds the case table
that tests/test_host_conv_exact.py (regime conditions, dispatch coverage) and tests/test_gpu_conv_exact.py (the sweep) share.

Conventions, as the HIP path stores things:
  y  = r16(act((conv(x, w) + b) * bn_scale + bn_shift) + residual)
  g  = r16(dy * act'(y))      act' read off the OUTPUT: ReLU o > 0, Leaky / PReLU o >= 0 (slope > 0), the subgradient the
                              kernels document (dsr_common.h); torch picks the other side at exactly 0
  dx = r16(dgrad(g)),  dw = wgrad(x, g) (fp32, exact),  db = sum g,  dprelu = sum dy * (y / slope) * (y < 0)
Exactness holds for: no activation, ReLU, Leaky / PReLU with slope 0.25 or 0.5, bn_scale a power of two, integer bn_shift /
residual / addend / bias.
"""
import functools
import importlib
import math

import torch

_L = importlib.import_module("deep-super-resolution_amd._lib")
BF16, F16 = _L.BF16, _L.F16
ACT_NONE, ACT_LEAKY, ACT_PRELU, ACT_RELU = _L.ACT_NONE, _L.ACT_LEAKY, _L.ACT_PRELU, _L.ACT_RELU
PAD_ZERO, PAD_REFLECT, PAD_REPLICATE = _L.PAD_ZERO, _L.PAD_REFLECT, _L.PAD_REPLICATE
DTYPES = {BF16: torch.bfloat16, F16: torch.float16}
EXACT_LIMIT = float(2 ** 24)


def r8(c):
    return (c + 7) // 8 * 8


# ----------------------------------------------------------------------------- number formats
def r16(t, dtype):
    """float64 -> the 16-bit storage type (round to nearest even) -> float64.  The input must be exact in fp32 (everything in
    this module is: integers and quarter-integers below 2^24), so the detour through fp32 rounds once."""
    t = t.to(torch.float64)
    f = t.to(torch.float32)
    assert torch.equal(f.to(torch.float64), t), "r16: value not exact in fp32"
    return f.to(DTYPES[dtype] if not isinstance(dtype, torch.dtype) else dtype).to(torch.float64)


def representable(t, dtype):
    return bool(torch.equal(r16(t, dtype), t.to(torch.float64)))


def tie_counts(t, dtype):
    """(ties rounded down in magnitude, ties rounded up in magnitude): values exactly half-way between two neighbours of the
    storage type.  t is a tie iff it is not representable and its mirror image about r16(t) is."""
    t = t.to(torch.float64)
    c = r16(t, dtype)
    o = 2 * t - c
    tie = (c != t) & (r16(o, dtype) == o)
    return int((tie & (c.abs() < t.abs())).sum()), int((tie & (c.abs() > t.abs())).sum())


# ----------------------------------------------------------------------------- operand generators
def ternary(gen, shape, density):
    """Values in {-1, 0, 1}; a fraction `density` of them non-zero."""
    nz = torch.rand(shape, generator=gen) < density
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (nz * sign).to(torch.float64)


def small_ints(gen, shape, amp, density=1.0):
    """Integers in [-amp, amp]; a fraction `density` of the positions kept, the rest zero."""
    v = torch.randint(-amp, amp + 1, shape, generator=gen)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=gen) < density)
    return v.to(torch.float64)


# ----------------------------------------------------------------------------- the convolution, as sums over taps
def _pad_index(size, pad, mode):
    """For padded coordinate p in [0, size + 2 pad): the source index and whether it exists (zero padding: it does not)."""
    i = torch.arange(-pad, size + pad)
    if mode == PAD_REFLECT:
        i = i.abs()
        i = torch.where(i > size - 1, 2 * (size - 1) - i, i)
    elif mode == PAD_REPLICATE:
        i = i.clamp(0, size - 1)
    valid = (i >= 0) & (i < size)
    return i.clamp(0, size - 1), valid


def out_size(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _taps(h, w, k, stride, pad, mode):
    oh, ow = out_size(h, w, k, stride, pad)
    iy, vy = _pad_index(h, pad, mode)
    ix, vx = _pad_index(w, pad, mode)
    for kh in range(k):
        ry = torch.arange(oh) * stride + kh
        for kw in range(k):
            rx = torch.arange(ow) * stride + kw
            yield kh, kw, iy[ry], vy[ry].to(torch.float64), ix[rx], vx[rx].to(torch.float64)


def _gather(x, ys, vy, xs, vx):
    return x[:, :, ys][:, :, :, xs] * vy.view(1, 1, -1, 1) * vx.view(1, 1, 1, -1)


def conv_fwd(x, w, stride, pad, mode):
    """x [N, Cin, H, W], w [Cout, Cin, k, k] float64 -> [N, Cout, OH, OW]."""
    n, _, h, wd = x.shape
    k = w.shape[-1]
    oh, ow = out_size(h, wd, k, stride, pad)
    y = torch.zeros(n, w.shape[0], oh, ow, dtype=torch.float64)
    for kh, kw, ys, vy, xs, vx in _taps(h, wd, k, stride, pad, mode):
        y += torch.einsum("nchw,oc->nohw", _gather(x, ys, vy, xs, vx), w[:, :, kh, kw])
    return y


def conv_dgrad(g, w, h, wd, stride, pad, mode):
    """Adjoint of conv_fwd with respect to x (the padding's adjoint included): g [N, Cout, OH, OW] -> [N, Cin, H, W]."""
    n = g.shape[0]
    k = w.shape[-1]
    dx = torch.zeros(n, w.shape[1], h, wd, dtype=torch.float64)
    for kh, kw, ys, vy, xs, vx in _taps(h, wd, k, stride, pad, mode):
        c = torch.einsum("nohw,oc->nchw", g, w[:, :, kh, kw]) * vy.view(1, 1, -1, 1) * vx.view(1, 1, 1, -1)
        rows = torch.zeros(n, w.shape[1], h, c.shape[-1], dtype=torch.float64).index_add_(2, ys, c)
        dx.index_add_(3, xs, rows)
    return dx


def conv_wgrad(x, g, k, stride, pad, mode):
    """Gradient of conv_fwd with respect to w: [Cout, Cin, k, k]."""
    _, _, h, wd = x.shape
    dw = torch.zeros(g.shape[1], x.shape[1], k, k, dtype=torch.float64)
    for kh, kw, ys, vy, xs, vx in _taps(h, wd, k, stride, pad, mode):
        dw[:, :, kh, kw] = torch.einsum("nohw,nchw->oc", g, _gather(x, ys, vy, xs, vx))
    return dw


def pixel_shuffle2(y):
    """nn.PixelShuffle(2): out[n, c, 2h + i, 2w + j] = y[n, 4c + 2i + j, h, w]."""
    n, c4, h, w = y.shape
    return y.view(n, c4 // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, c4 // 4, 2 * h, 2 * w)


def pixel_unshuffle2(y):
    n, c, h2, w2 = y.shape
    return y.view(n, c, h2 // 2, 2, w2 // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(n, 4 * c, h2 // 2, w2 // 2)


def act_fwd(z, act, slope):
    if act == ACT_NONE:
        return z
    if act == ACT_RELU:
        return z.clamp_min(0)
    return torch.where(z >= 0, z, z * slope)


def act_grad_from_out(o, act, slope):
    if act == ACT_NONE:
        return torch.ones_like(o)
    if act == ACT_RELU:
        return (o > 0).to(torch.float64)
    return torch.where(o >= 0, 1.0, slope).to(torch.float64)


# ----------------------------------------------------------------------------- the case table
ACTS = {"none": ACT_NONE, "leaky": ACT_LEAKY, "prelu": ACT_PRELU, "relu": ACT_RELU}
PERSIST, T16, T64, T128, T64x128, T256, T224 = ("conv_gemm_persist_kernel", "conv_gemm_kernel<128x16>", "conv_gemm_kernel<128x64>",
                                                "conv_gemm_kernel<128x128>", "conv_gemm_kernel<64x128>",
                                                "conv_gemm_kernel<256x256>", "conv_gemm_kernel<224x256>")
C64_0, C64_1, C64_2, C64_3 = ("conv_c64_kernel<%d>" % i for i in range(4))
HALO, CIN8, RGB9, SMALLN, TOEP9, DS2 = ("conv_halo64_kernel", "conv_cin8_kernel", "conv_rgb9_kernel", "conv_smalln_kernel",
                                        "conv_dgrad_toeplitz9_kernel", "conv_dgrad_s2_kernel")
W_DMA, W_S2, W_1X1, W_TAPS, W_TOEP, W_RGB9, W_GEN = ("conv_wgrad_dma_kernel", "conv_wgrad_dma_s2_kernel", "conv_wgrad_tile_kernel<1x1>",
                                                      "conv_wgrad_taps_kernel", "conv_wgrad_toeplitz9_kernel", "conv_rgb9_wgrad_kernel",
                                                      "conv_wgrad_kernel")
ALL_KERNEL_NAMES = {C64_0, C64_1, C64_2, C64_3, HALO, CIN8, RGB9, SMALLN, TOEP9, DS2, PERSIST, T16, T64, T128, T64x128, T256, T224,
                    W_DMA, W_S2, W_1X1, W_TAPS, W_TOEP, W_RGB9, W_GEN}
HALO2 = {"DSR_CONV_HALO64": "2"}
S2_ONE = {"DSR_DGRAD_S2": "2"}          # the single-launch stride-2 input gradient however small the grid
S2_FOUR = {"DSR_DGRAD_S2": "0"}         # four parity-class launches of the gather kernel
BIG256 = {"DSR_CONV_BIG_TILES": "1", "DSR_CONV_BM224": "0"}
BIG224 = {"DSR_CONV_BIG_TILES": "1", "DSR_CONV_BM224": "2"}


def case(name, n, cin, cout, h, w, k, stride, pad, names, mode=PAD_ZERO, act="none", slope=0.25, bias=True, stats=False, ps=False,
         nchw=False, fold=False, residual=False, dgrad="plain", env=None, dens=0.3, regime_b=False):
    """names = (forward, input gradient, weight gradient) kernel as dsr_conv_kernel_name must report it under `env` with this
    case's epilogue.  dgrad: "plain" | "add" (dsr_conv_dgrad_add) | "relu" / "leaky" (dsr_conv_dgrad_masked) | None (not
    available: replicate padding)."""
    return dict(name=name, n=n, cin=cin, cout=cout, h=h, w=w, k=k, stride=stride, pad=pad, names=names, mode=mode, act=ACTS[act],
                slope=slope, bias=bias, stats=stats, ps=ps, nchw=nchw, fold=fold, residual=residual or fold, dgrad=dgrad,
                env=env or {}, dens=dens, regime_b=regime_b)


CASES = [
    # ---- conv_c64_kernel<0..3>: 64 -> 64 3x3 s1 p1, and the wide form
    case("c64_one_ragged_tile", 2, 64, 64, 7, 9, 3, 1, 1, (C64_1, C64_1, W_DMA), act="leaky"),
    case("c64_tiles_ragged_right", 2, 64, 64, 12, 37, 3, 1, 1, (C64_1, C64_1, W_DMA), regime_b=True),
    case("c64_stats", 2, 64, 64, 12, 37, 3, 1, 1, (C64_0, C64_1, W_DMA), stats=True),
    case("c64_stats_one_tile", 2, 64, 64, 7, 9, 3, 1, 1, (C64_0, C64_1, W_DMA), stats=True, dgrad="add"),
    case("c64_fold_residual_prelu", 2, 64, 64, 12, 37, 3, 1, 1, (C64_2, C64_1, W_DMA), act="prelu", fold=True, dens=0.15,
         dgrad="relu"),
    case("c64_residual_only", 2, 64, 64, 7, 9, 3, 1, 1, (C64_3, C64_1, W_DMA), residual=True, dgrad="leaky"),
    case("c64_wide_192", 2, 64, 192, 12, 37, 3, 1, 1, (C64_1, HALO, W_DMA), act="relu"),
    case("c64_wide_256_pixel_shuffle", 2, 64, 256, 7, 9, 3, 1, 1, (C64_1, T64, W_DMA), act="prelu", ps=True),
    case("c64_wide_128_stats", 1, 64, 128, 12, 37, 3, 1, 1, (C64_0, HALO, W_DMA), stats=True),
    # ---- conv_halo64_kernel: forward (two 64-channel slices) and mirrored input gradient, plain and masked
    case("halo64_fwd_128", 1, 128, 128, 8, 32, 3, 1, 1, (HALO, HALO, W_DMA), env=HALO2, act="relu"),
    case("halo64_fwd_256_128", 1, 256, 128, 19, 45, 3, 1, 1, (HALO, T64x128, W_DMA), env=HALO2, act="leaky", regime_b=True),
    case("halo64_dgrad_128", 1, 64, 128, 16, 64, 3, 1, 1, (C64_1, HALO, W_DMA), dgrad="leaky"),
    case("halo64_dgrad_256_ragged", 2, 64, 256, 21, 75, 3, 1, 1, (C64_1, HALO, W_DMA), act="leaky", regime_b=True),
    # ---- conv_cin8_kernel forward, conv_smalln_kernel (flip) input gradient
    case("cin8_rgb", 2, 3, 64, 16, 24, 3, 1, 1, (CIN8, SMALLN, W_DMA), act="leaky"),
    case("cin8_gray_ragged", 3, 1, 64, 37, 70, 3, 1, 1, (CIN8, SMALLN, W_DMA), act="relu", regime_b=True),
    # ---- conv_rgb9_kernel forward and weight gradient, small-N 9x9 (flip) input gradient
    case("rgb9_gray_small_map", 1, 1, 64, 9, 33, 9, 1, 4, (RGB9, SMALLN, W_RGB9), act="leaky"),
    case("rgb9_rgb_ragged", 3, 3, 64, 37, 45, 9, 1, 4, (RGB9, SMALLN, W_RGB9), act="prelu", regime_b=True),
    # ---- small-N forward / Toeplitz: the 9x9 tail, few outputs, fp32 NCHW output
    case("tail9_12", 1, 64, 3, 12, 12, 9, 1, 4, (SMALLN, TOEP9, W_TOEP)),
    case("tail9_16", 2, 64, 3, 16, 16, 9, 1, 4, (SMALLN, TOEP9, W_TOEP)),
    case("tail9_ragged_strips", 2, 64, 3, 75, 140, 9, 1, 4, (SMALLN, TOEP9, W_TOEP), regime_b=True, dens=0.2),
    case("tail9_70x130", 1, 64, 3, 70, 130, 9, 1, 4, (SMALLN, TOEP9, W_TOEP), dens=0.2),
    case("smalln_64_4_3x3", 2, 64, 4, 12, 12, 3, 1, 1, (SMALLN, T64, W_DMA), act="leaky"),
    case("t16_32_4_3x3", 2, 32, 4, 12, 12, 3, 1, 1, (T16, T64, W_DMA)),
    case("smalln_nchw_cout3", 2, 64, 3, 9, 11, 9, 1, 4, (SMALLN, TOEP9, W_TOEP), nchw=True),
    case("smalln_nchw_cout5", 2, 64, 5, 9, 11, 3, 1, 1, (SMALLN, T64, W_DMA), nchw=True),
    # ---- 3x3 stride 2: conv_dgrad_s2_kernel, the four-launch form (odd sizes: unequal parity classes), dma_s2 weight gradient
    case("s2_64_64", 2, 64, 64, 16, 16, 3, 2, 1, (T64, DS2, W_S2), env=S2_ONE, act="leaky"),
    case("s2_64_128_odd", 1, 64, 128, 15, 17, 3, 2, 1, (T64x128, T64, W_S2)),
    case("s2_128_192", 1, 128, 192, 50, 38, 3, 2, 1, (T128, DS2, W_S2), env=S2_ONE, regime_b=True),
    case("s2_128_192_four_launches", 1, 128, 192, 50, 38, 3, 2, 1, (T128, T64x128, W_S2), env=S2_FOUR),
    case("s2_64_128_wgrad_chunks", 2, 64, 128, 33, 70, 3, 2, 1, (T64x128, T64, W_S2)),
    # ---- the gather kernel's tiles and padding modes
    case("persist_1x1_64_64", 3, 64, 64, 256, 256, 1, 1, 0, (PERSIST, PERSIST, W_1X1), act="relu", dens=0.2),
    case("t16_1x1_reflect", 1, 32, 4, 12, 12, 1, 1, 0, (T16, T64, W_1X1), mode=PAD_REFLECT),
    case("t64_128_64", 1, 128, 64, 9, 11, 3, 1, 1, (T64, T64x128, W_DMA), act="leaky"),
    case("t128_reflect_132", 1, 132, 128, 10, 12, 3, 1, 1, (T128, T128, W_DMA), mode=PAD_REFLECT),
    case("t128_reflect_dma_128", 2, 128, 128, 13, 19, 3, 1, 1, (T128, T64x128, W_DMA), mode=PAD_REFLECT, act="leaky", regime_b=True),
    case("t64_reflect_64_128", 1, 64, 128, 12, 20, 3, 1, 1, (T128, T64, W_DMA), mode=PAD_REFLECT, regime_b=True),
    case("t128_reflect_s2_132", 1, 132, 128, 16, 18, 3, 2, 1, (T128, T128, W_S2), mode=PAD_REFLECT),
    case("t128_reflect_s2_128", 1, 128, 128, 16, 18, 3, 2, 1, (T128, T64x128, W_S2), mode=PAD_REFLECT),
    case("t128_replicate", 1, 128, 128, 9, 11, 3, 1, 1, (T128, None, None), mode=PAD_REPLICATE, dgrad=None),
    case("t64x128_1x1_128", 2, 128, 128, 8, 8, 1, 1, 0, (T64x128, T64x128, W_1X1), act="leaky"),
    case("t64x128_forced", 1, 128, 128, 9, 11, 3, 1, 1, (T64x128, T64x128, W_DMA), env={"DSR_CONV_BM64": "2"}),
    case("t128_bm64_off", 1, 128, 128, 9, 11, 3, 1, 1, (T128, T128, W_DMA), env={"DSR_CONV_BM64": "0"}, dgrad="relu"),
    case("t256_128_256", 1, 128, 256, 8, 8, 3, 1, 1, (T256, T64x128, W_DMA), env=BIG256, act="relu"),
    case("t224_256_256", 1, 256, 256, 8, 8, 3, 1, 1, (T224, T224, W_DMA), env=BIG224),
    # ---- weight gradients: two 64-channel blocks each way, the 9x9 taps kernel, generic split-K
    case("wgrad_dma_192_384", 1, 192, 384, 9, 11, 3, 1, 1, (T64x128, T128, W_DMA)),
    case("wgrad_dma_64_64_chunks", 2, 64, 64, 40, 40, 3, 1, 1, (C64_1, C64_1, W_DMA)),
    case("wgrad_taps_9x9_16_8", 2, 16, 8, 20, 37, 9, 1, 4, (T16, T16, W_TAPS)),
    case("wgrad_generic_9x9_reflect", 2, 16, 16, 20, 20, 9, 1, 4, (T16, T16, W_GEN), mode=PAD_REFLECT),
    case("wgrad_generic_stride3", 2, 64, 64, 40, 40, 3, 3, 1, (T64, T64, W_GEN)),
]
CASE_IDS = [c["name"] for c in CASES]


def kernel_names(lib, c, dtype=BF16):
    """(forward, dgrad, wgrad) names the dispatcher plans for case c with its own epilogue; the caller sets c["env"]."""
    import ctypes as C
    d = _L.ConvDesc(dtype, c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"], c["k"], c["stride"], c["pad"], c["mode"])
    dummy = (C.c_float * 4)()
    a = C.addressof(dummy)
    ep = _L.Epilogue(c["act"], c["slope"], a if c["act"] == ACT_PRELU else None, a if c["bias"] else None, a if c["stats"] else None,
                     int(c["ps"]), a if c["nchw"] else None, a if c["fold"] else None, a if c["fold"] else None,
                     a if c["residual"] else None)
    return tuple(lib.dsr_conv_kernel_name(C.byref(d), op, C.byref(ep) if op == 0 else None).decode() for op in (0, 1, 2))


# ----------------------------------------------------------------------------- one layer, forward and backward
def _seed(c, salt=0):
    return 1000 * sum(ord(ch) for ch in c["name"]) + salt


@functools.lru_cache(maxsize=None)
def layer_a(name):
    """Regime A (no rounding anywhere): operands and every expected tensor of case `name`, all float64 NCHW / OIHW.  Computed
    once and shared; callers must not modify it."""
    c = CASES[CASE_IDS.index(name)]
    gen = torch.Generator().manual_seed(_seed(c))
    n, cin, cout, h, w, k, st, pad, mode = (c[q] for q in ("n", "cin", "cout", "h", "w", "k", "stride", "pad", "mode"))
    p = c["dens"]
    r = dict(case=c)
    r["x"] = ternary(gen, (n, cin, h, w), p)
    r["w"] = ternary(gen, (cout, cin, k, k), p)
    r["b"] = small_ints(gen, (cout,), 3) if c["bias"] else None
    conv = conv_fwd(r["x"], r["w"], st, pad, mode)
    r["bound_fwd"] = float(conv_fwd(r["x"].abs(), r["w"].abs(), st, pad, mode).max()) + 3
    z = conv + (r["b"].view(1, -1, 1, 1) if c["bias"] else 0)
    r["stats"] = torch.stack([z.sum(dim=(0, 2, 3)), (z * z).sum(dim=(0, 2, 3))])          # pre-activation sums, per channel
    r["bound_stats"] = float((z * z).sum(dim=(0, 2, 3)).max())
    inter = [z]
    if c["fold"]:
        r["bn_scale"] = 2.0 ** torch.randint(0, 2, (cout,), generator=gen).to(torch.float64)
        r["bn_shift"] = small_ints(gen, (cout,), 4)
        z = z * r["bn_scale"].view(1, -1, 1, 1) + r["bn_shift"].view(1, -1, 1, 1)
        inter.append(z)
    a = act_fwd(z, c["act"], c["slope"])
    inter.append(a)
    if c["residual"]:
        r["residual"] = small_ints(gen, tuple(a.shape), 5)
        a = a + r["residual"]
    r["y"] = a                                              # [N, Cout, OH, OW]; the pixel-shuffled view is pixel_shuffle2(y)
    r["inter"] = inter
    # backward: dy arrives in the layout of the stored output; the activation's derivative is read off that output
    r["dy"] = ternary(gen, tuple(a.shape), p)
    o = inter[-1] if not c["residual"] else None
    if c["residual"] or c["nchw"]:
        g = r["dy"]                                         # the raw-ABI backward of these epilogues starts from g itself
    else:
        g = r["dy"] * act_grad_from_out(o, c["act"], c["slope"])
        if c["act"] == ACT_PRELU:
            r["dprelu"] = (r["dy"] * (o / c["slope"]) * (o < 0)).sum()
            r["bound_dprelu"] = float((r["dy"] * (o / c["slope"]) * (o < 0)).abs().sum())
    r["g"] = g
    r["db"] = g.sum(dim=(0, 2, 3))
    r["bound_db"] = float(g.abs().sum(dim=(0, 2, 3)).max())
    if c["dgrad"] is not None:
        r["dx_plain"] = conv_dgrad(g, r["w"], h, w, st, pad, mode)
        r["bound_dgrad"] = float(conv_dgrad(g.abs(), r["w"].abs(), h, w, st, pad, mode).max())
        dx = r["dx_plain"]
        if c["dgrad"] == "add":
            r["addend"] = small_ints(gen, tuple(dx.shape), 5)
            dx = dx + r["addend"]
        elif c["dgrad"] in ("relu", "leaky"):
            # x_act: the conv's own input seen as the output of the activation in front of it
            r["mask_act"] = ACT_RELU if c["dgrad"] == "relu" else ACT_LEAKY
            dx = dx * act_grad_from_out(r["x"], r["mask_act"], 0.25)
        r["dx"] = dx
    if c["names"][2] is not None:
        r["dw"] = conv_wgrad(r["x"], g, k, st, pad, mode)
        r["bound_wgrad"] = float(conv_wgrad(r["x"].abs(), g.abs(), k, st, pad, mode).max())
    return r


B_SIGMA = {BF16: 300.0, F16: 2500.0}     # spread of the outputs: bf16 rounds integers above 256, fp16 above 2048


def _amp(sigma, terms, other):
    """Amplitude a such that sum of `terms` products of uniform integers in [-a, a] x [-other, other] has about this sigma."""
    return max(1, min(200, int(round(3.0 * sigma / (math.sqrt(terms) * other)))))


@functools.lru_cache(maxsize=None)
def layer_b(name, dtype):
    """Regime B (rounding exercised): dense operands scaled so that the outputs leave the exactly representable range of
    `dtype`; no bias, no activation.  Expected: r16 of the exact result, forward and input gradient."""
    c = CASES[CASE_IDS.index(name)]
    gen = torch.Generator().manual_seed(_seed(c, 7 + dtype))
    n, cin, cout, h, w, k, st, pad, mode = (c[q] for q in ("n", "cin", "cout", "h", "w", "k", "stride", "pad", "mode"))
    kf = cin * k * k
    kd = max(1, cout * k * k // (st * st))
    aw = max(1, int(round(math.sqrt(3.0 * B_SIGMA[dtype] / math.sqrt(kf)))))
    ax, ag = _amp(B_SIGMA[dtype], kf, aw), _amp(B_SIGMA[dtype], kd, aw)
    r = dict(case=c, amps=(ax, aw, ag))
    r["x"] = small_ints(gen, (n, cin, h, w), ax)
    r["w"] = small_ints(gen, (cout, cin, k, k), aw)
    r["y_exact"] = conv_fwd(r["x"], r["w"], st, pad, mode)
    r["bound_fwd"] = float(conv_fwd(r["x"].abs(), r["w"].abs(), st, pad, mode).max())
    r["y"] = r16(r["y_exact"], dtype)
    r["g"] = small_ints(gen, tuple(r["y"].shape), ag)
    r["dx_exact"] = conv_dgrad(r["g"], r["w"], h, w, st, pad, mode)
    r["bound_dgrad"] = float(conv_dgrad(r["g"].abs(), r["w"].abs(), h, w, st, pad, mode).max())
    r["dx"] = r16(r["dx_exact"], dtype)
    return r


WGRAD_SCRATCH_SLABS = 16          # DSR_WGRAD_SCRATCH_SLABS (csrc/dsr_kernels.h): slabs the reduction keeps behind the partial ones


def wgrad_slabs(lib, c, dtype=BF16):
    """Partial slabs (ychunks / splits) the weight gradient of case c is reduced over (not defined for the rgb9 kernel)."""
    import ctypes as C
    d = _L.ConvDesc(dtype, c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"], c["k"], c["stride"], c["pad"], c["mode"])
    slab = c["k"] * c["k"] * r8(c["cin"]) * r8(c["cout"]) * 4
    return lib.dsr_conv_wgrad_workspace(C.byref(d)) // slab - WGRAD_SCRATCH_SLABS
