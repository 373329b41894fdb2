"""Float64 CPU yardstick of the SRVGGNetCompact path (models/GAN/srvgg.py, csrc/conv_compact.hip, csrc/pw_compact.hip).

A restatement with F.conv2d, F.prelu, F.pixel_shuffle and F.interpolate(mode='nearest') of
  * one body launch (dsr_conv_prelu_c_fwd):   v = conv3x3(x, w) + b;  v = v > 0 ? v : v * slope[c];  y = r16(v)
  * one tail launch (dsr_conv_shuffle_add_fwd):  pixel_shuffle(conv3x3(x, w) + b, s) + nearest_s(base), fp32, no rounding
  * the pointwise PReLU backward in closed form and the shuffle-add pair,
  * the whole network, written from BasicSR's published definition (no package and no trained weights were available: parity
    with BasicSR is unpinned; this file is what the HIP path is held to),
with an optional STORAGE MODEL that rounds to the 16-bit type exactly where each form of the HIP path stores a 16-bit tensor
(fused=False also rounds the pre-activation z of every body layer; the head stores z in both forms), the state_dict key /
shape table, and the exact-integer operand generators of the single-launch sweep.  Nothing is imported from the package
under test but _lib's constants (through conv_exact_ref).
"""
import math

import torch
import torch.nn.functional as TF

from conv_exact_ref import BF16, DTYPES, F16, r16, representable, small_ints, ternary  # noqa: F401

LEAKY = 0.1
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))       # a host float as the kernels receive it


# ----------------------------------------------------------------------------- keys and shapes
def key_table(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"):
    """[(state_dict key, shape)] in BasicSR's order."""
    out = []
    last = 2 * num_conv + 2
    for i in range(0, last + 1, 2):
        cout = num_feat if i < last else num_out_ch * upscale * upscale
        out.append((f"body.{i}.weight", (cout, num_in_ch if i == 0 else num_feat, 3, 3)))
        out.append((f"body.{i}.bias", (cout,)))
        if act_type == "prelu" and i < last:
            out.append((f"body.{i + 1}.weight", (num_feat,)))
    return out


def param_count(**kw):
    return sum(math.prod(s) for _, s in key_table(**kw))


def template(**kw):
    return {k: torch.zeros(s) for k, s in key_table(**kw)}


# ----------------------------------------------------------------------------- single launches
def prelu_c(v, slope):
    """v [N, C, H, W], slope [C]: torch's PReLU (the branch v > 0; 0 takes the slope side, where both sides agree)."""
    return torch.where(v > 0, v, v * slope.double().view(1, -1, 1, 1))


def conv_prelu(x, w, b, slope):
    """Unrounded float64 value of one body launch.  b, slope: [Cout] or None (slope None: no activation)."""
    v = TF.conv2d(x.double(), w.double(), None, 1, 1)
    if b is not None:
        v = v + b.double().view(1, -1, 1, 1)
    return v if slope is None else prelu_c(v, slope)


def conv_abs(x, w, b):
    """A = sum |x| |w| + |b| per output."""
    a = TF.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    return a if b is None else a + b.double().abs().view(1, -1, 1, 1)


def body_bound(y64, x, w, b, slope, dtype):
    """|y - y64| <= u |y64| + (9 * 64 + 4) 2^-24 A max(1, |slope_c|): 9 * 64 + 4 fp32 operations of relative error 2^-24 on
    magnitudes bounded by A (times |slope| behind the activation), then one rounding to 16 bits (u: one ulp of the type)."""
    u = 2.0 ** -8 if dtype == BF16 else 2.0 ** -10
    amp = 1.0 if slope is None else slope.double().abs().clamp_min(1.0).view(1, -1, 1, 1)
    return u * y64.abs() + (9 * 64 + 4) * 2.0 ** -24 * conv_abs(x, w, b) * amp


def shuffle(t, s, swap=False):
    """PixelShuffle(s): out[n, c, s y + i, s x + j] = t[n, c s^2 + i s + j, y, x].  swap=True: i and j exchanged (the mistake
    the bounds must catch)."""
    n, q, h, w = t.shape
    c = q // (s * s)
    v = t.view(n, c, s, s, h, w)
    if swap:
        v = v.transpose(2, 3)
    return v.permute(0, 1, 4, 2, 5, 3).reshape(n, c, s * h, s * w)


def nearest(x, s):
    return x if s == 1 else TF.interpolate(x, scale_factor=s, mode="nearest")


def shuffle_add(t, base, s, swap=False):
    out = shuffle(t.double(), s, swap)
    return out if base is None else out + nearest(base.double(), s)


def conv_tail(x, w, b, base, s, swap=False):
    """Unrounded float64 value of one tail launch: [N, C, sH, sW]."""
    return shuffle_add(conv_prelu(x, w, b, None), base, s, swap)


def tail_bound(x, w, b, base, s):
    """|out - out64| <= (9 * 64 + 3) 2^-24 (A + |base|), no 16-bit term."""
    a = shuffle(conv_abs(x, w, b), s)
    if base is not None:
        a = a + nearest(base.double().abs(), s)
    return (9 * 64 + 3) * 2.0 ** -24 * a


def shuffle_add_bwd(dout, s):
    """(dt, dbase) of shuffle_add: the un-shuffle of dout, and its s^2-pixel sums."""
    n, c, sh, sw = dout.shape
    h, w = sh // s, sw // s
    v = dout.double().view(n, c, h, s, w, s)
    return v.permute(0, 1, 3, 5, 2, 4).reshape(n, c * s * s, h, w), v.sum(dim=(3, 5))


def prelu_bwd(dy, z, slope, from_output=False):
    """Closed form of torch's PReLU backward on [N, C, H, W]: dz = dy (z > 0 ? 1 : slope_c), dslope_c = sum dy z [z <= 0].
    from_output=True: the branch taken from the OUTPUT prelu_c(z) instead (the mistake the bounds must catch: wrong for a
    negative slope, where a negative z has a positive output)."""
    dy, z = dy.double(), z.double()
    sl = slope.double().view(1, -1, 1, 1)
    key = prelu_c(z, slope) if from_output else z
    pos = key > 0
    src = torch.where(pos, torch.zeros_like(z), z if not from_output else key / torch.where(sl == 0, torch.ones_like(sl), sl))
    return torch.where(pos, dy, dy * sl), (dy * src).sum(dim=(0, 2, 3))


def exact_slopes(c=64, shift=0):
    """Per-channel slopes from {0, +-2^k}, k in -2..1, all different from their neighbours: a channel mix-up or a sign
    assumption changes the result.  shift: rolled by that many channels."""
    vals = torch.tensor([0.25, -0.5, 0.0, 2.0, -0.25, 0.5, -1.0, 1.0, -2.0], dtype=torch.float64)
    return vals[(torch.arange(c) + shift) % len(vals)]


def exact_body(n, h, w, seed=0):
    """(x [N,64,H,W] ints in [-3, 3], ternary w of density 0.25, integer bias in [-4, 4], slopes): every fp32 sum is exact
    and every result representable in bf16 and fp16."""
    g = torch.Generator().manual_seed(1000 * n + 100 * h + 10 * w + seed)
    return small_ints(g, (n, 64, h, w), 3), ternary(g, (64, 64, 3, 3), 0.25), small_ints(g, (64,), 4), exact_slopes()


def exact_tail(n, h, w, s, c=3, seed=0):
    """(x, w [c s^2,64,3,3], bias [c s^2], base [N,c,H,W]) in integers."""
    g = torch.Generator().manual_seed(1000 * n + 100 * h + 10 * w + s + seed)
    q = c * s * s
    return (small_ints(g, (n, 64, h, w), 3), ternary(g, (q, 64, 3, 3), 0.25), small_ints(g, (q,), 4),
            small_ints(g, (n, c, h, w), 9))


EXACT_SHAPES = [(1, 8, 64, 0), (2, 9, 65, 0), (1, 3, 5, 0), (1, 16, 130, 2)]   # (N, H, W, max_blocks)
CAP_SHAPE = (65, 9, 65)                # 65 images of 4 ragged tiles = 260 work items on the launcher's cap of 256 blocks
GRID_CAP = 256
FLOAT_PARTITIONS = (0, 1, 3)


def tiles(n, h, w):
    return n * -(-h // 8) * -(-w // 64)


def float_body(dtype, n=2, h=9, w=65, seed=0):
    """N(0, 1) data, N(0, 0.05) weights, slopes in [-1.5, 1.5] (some negative, some above one)."""
    g = torch.Generator().manual_seed(77 + seed)
    t16 = lambda t: t.to(DTYPES[dtype]).double()
    x = t16(torch.randn(n, 64, h, w, generator=g, dtype=torch.float64))
    wt = t16(torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05)
    bias = (torch.randn(64, generator=g, dtype=torch.float64) * 0.1).float().double()
    slope = ((torch.rand(64, generator=g, dtype=torch.float64) * 3.0 - 1.5)).float().double()
    return x, wt, bias, slope


def float_tail(dtype, s, n=2, h=9, w=65, c=3):
    g = torch.Generator().manual_seed(91 + s)
    t16 = lambda t: t.to(DTYPES[dtype]).double()
    q = c * s * s
    x = t16(torch.randn(n, 64, h, w, generator=g, dtype=torch.float64))
    wt = t16(torch.randn(q, 64, 3, 3, generator=g, dtype=torch.float64) * 0.05)
    bias = (torch.randn(q, generator=g, dtype=torch.float64) * 0.1).float().double()
    base = torch.rand(n, c, h, w, generator=g, dtype=torch.float64).float().double()
    return x, wt, bias, base


# ----------------------------------------------------------------------------- the network
def _store(t, dtype):
    """Storage model: float64 -> fp32 -> the 16-bit type -> float64 (None: no rounding)."""
    if dtype is None:
        return t
    return t.to(torch.float32).to(DTYPES[dtype] if not isinstance(dtype, torch.dtype) else dtype).to(torch.float64)


def network(sd, x, upscale, dtype=None, fused=True, act=None):
    """SRVGGNetCompact forward in float64 from a state_dict (num_conv and the widths are read off the keys) and an fp32 NCHW
    input.  The activation is PReLU when the state_dict holds ``body.1.weight``; otherwise `act` says 'relu' or 'leakyrelu'.
    dtype=None: pure float64.  Otherwise the storage model of the HIP path: the 16-bit weight images, the 16-bit input copy
    and every 16-bit activation tensor are rounded where that path stores them -- fused: one rounding per body layer,
    r16(prelu(v)); composed (fused=False): also the pre-activation, r16(prelu(r16(v))).  The head stores its pre-activation in
    both forms.  The tail and the added input image stay in fp32 / float64: no rounding."""
    st = lambda t: _store(t, dtype)
    last = max(int(k.split(".")[1]) for k in sd if k.endswith(".bias"))
    nf = sd["body.0.weight"].shape[0]
    x = x.double()

    def slope(i):
        if f"body.{i}.weight" in sd:
            return sd[f"body.{i}.weight"].double()
        if act not in ("relu", "leakyrelu"):
            raise ValueError("network: no PReLU keys; say act='relu' or act='leakyrelu'")
        return torch.full((nf,), 0.0 if act == "relu" else F32(LEAKY), dtype=torch.float64)

    def prelu(v, i):
        return TF.prelu(v, slope(i))

    conv = lambda v, i: TF.conv2d(v, st(sd[f"body.{i}.weight"].double()), sd[f"body.{i}.bias"].double(), 1, 1)
    feat = st(prelu(st(conv(st(x), 0)), 1))
    for i in range(2, last, 2):
        v = conv(feat, i)
        if not (fused or dtype is None):
            v = st(v)
        feat = st(prelu(v, i + 1))
    return TF.pixel_shuffle(conv(feat, last), upscale) + nearest(x, upscale)
