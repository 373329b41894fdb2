"""Float64 CPU yardstick of the RRDBNet path (models/GAN/rrdbnet.py, csrc/conv_rdb.hip).

A restatement with F.conv2d, torch.cat and F.interpolate(mode='nearest') of
  * one prefix-convolution launch over a growth buffer (dsr_conv_rdb_fwd):
        v = conv3x3(x[:, :Cin], w) + b;  v = act(v);  v = v * beta1 + res1;  v = v * beta2 + res2;  y = r16(v)
  * the whole network, written from BasicSR's published definition (no package and no trained weights were available:
    parity with BasicSR is unpinned; this file is what the HIP path is held to),
with an optional STORAGE MODEL that rounds to the 16-bit type exactly where the HIP path stores a 16-bit tensor (and rounds
the weights, which the kernels read from 16-bit images), the state_dict key / shape table, and the exact-integer operand
generators of the single-launch sweep.  Nothing is imported from the package under test but _lib's constants (through
conv_exact_ref).
"""
import math

import torch
import torch.nn.functional as TF

from conv_exact_ref import BF16, DTYPES, F16, conv_fwd, r16, representable, small_ints, ternary  # noqa: F401

SLOPE, BETA = 0.2, 0.2
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))       # a host float as the kernels receive it


# ----------------------------------------------------------------------------- keys and shapes
def key_table(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
    """[(state_dict key, shape)] in BasicSR's order."""
    u = {4: 1, 2: 2, 1: 4}[scale]
    out = []

    def conv(name, cout, cin):
        out.append((name + ".weight", (cout, cin, 3, 3)))
        out.append((name + ".bias", (cout,)))

    conv("conv_first", num_feat, num_in_ch * u * u)
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in range(5):
                conv(f"body.{i}.rdb{j}.conv{k + 1}", num_grow_ch if k < 4 else num_feat, num_feat + k * num_grow_ch)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, num_feat, num_feat)
    conv("conv_last", num_out_ch, num_feat)
    return out


def param_count(**kw):
    return sum(math.prod(s) for _, s in key_table(**kw))


def template(**kw):
    return {k: torch.zeros(s) for k, s in key_table(**kw)}


# ----------------------------------------------------------------------------- one launch
def prefix_conv(x, w, b, slope=None, res1=None, beta1=0.0, res2=None, beta2=0.0, taps=False):
    """Unrounded float64 value of one launch.  x [N, Cin, H, W] (the prefix), w [Cout, Cin, 3, 3], b [Cout] or None, res*
    [N, Cout, H, W] or None; slope=None: no activation.  taps=True: the sum over taps of conv_exact_ref instead of F.conv2d."""
    x, w = x.double(), w.double()
    v = conv_fwd(x, w, 1, 1, 0) if taps else TF.conv2d(x, w, None, 1, 1)
    if b is not None:
        v = v + b.double().view(1, -1, 1, 1)
    if slope is not None:
        v = torch.where(v >= 0, v, v * slope)
    if res1 is not None:
        v = v * beta1 + res1.double()
    if res2 is not None:
        v = v * beta2 + res2.double()
    return v


def prefix_conv_bound(x, w, b, cin, res1=None, beta1=0.0, res2=None, beta2=0.0):
    """A of the float-data bound |y - y64| <= u |y64| + (9 Cin + 4) 2^-24 A:  conv(|x|, |w|) + |b|, carried through the
    residual steps with absolute values."""
    a = TF.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    if b is not None:
        a = a + b.double().abs().view(1, -1, 1, 1)
    if res1 is not None:
        a = a * abs(beta1) + res1.double().abs()
    if res2 is not None:
        a = a * abs(beta2) + res2.double().abs()
    return a


def exact_operands(seed, n, h, w, cin, cout, amp=3, res=0):
    """The integer operands of the single-launch sweep: x in [-amp, amp] on all 192 channels of a growth buffer (NCHW here),
    ternary weights of density 0.25, integer bias in [-4, 4], `res` integer residuals in [-3, 3] on 192 channels each."""
    g = torch.Generator().manual_seed(seed)
    buf = small_ints(g, (n, 192, h, w), amp)
    wt = ternary(g, (cout, cin, 3, 3), 0.25)
    bias = small_ints(g, (cout,), 4)
    residuals = [small_ints(g, (n, 192, h, w), 3) for _ in range(res)]
    return buf, wt, bias, residuals


EXACT_CASES = [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64)]          # (Cin, Cout) of the five launches of a block
EXACT_SHAPES = [(1, 8, 64, 0), (2, 9, 65, 0), (1, 3, 5, 0), (1, 16, 130, 2)]   # (N, H, W, max_blocks)
EXACT_SLOPE = EXACT_BETA = 0.25
R2_OFF = 64        # the second residual is read at this channel offset of its own buffer (the first at 0 of the input buffer)


# the launcher's work partition (csrc/conv_rdb.hip), restated: a work item of the forward is one 8 x 64 pixel tile of one image,
# the grid is min(items, max_blocks or 256) blocks, and block b takes the items b, b + blocks, b + 2 blocks, ...
RDB_GRID_CAP = 256
CAP_SHAPE = (65, 9, 65)                # 65 images of 4 ragged tiles = 260 items: past the natural cap, no max_blocks
FLOAT_PARTITIONS = (0, 1, 3)           # max_blocks of the partition-independence test on float data at (2, 9, 65), 8 items
FLOAT_PARTITION_CASES = [(96, 32, 0), (128, 32, 0), (192, 64, 1), (192, 64, 2)]      # 3 | 4 | 6 K-blocks: both parities


def rdb_tiles(n, h, w):
    return n * -(-h // 8) * -(-w // 64)


def fwd_plan(n, h, w, max_blocks=0):
    """(work items, blocks) of one forward launch."""
    items = rdb_tiles(n, h, w)
    return items, min(items, max_blocks if max_blocks > 0 else RDB_GRID_CAP)


def exact_launch(n, h, w, cin, cout, nres, amp=3):
    """One launch of the sweep as the GPU test issues it: (buf, wt, bias, res2 buffer or None, keyword arguments of
    prefix_conv).  Cout = 32: LeakyReLU(0.25), in place.  Cout = 64: no activation, res1 = channels [0, 64) of the input
    buffer itself (integers in [-amp, amp]), with nres = 2 also res2 = channels [64, 128) of a second buffer."""
    seed = 1000 * n + 100 * h + 10 * w + cin + nres + amp
    buf, wt, bias, res = exact_operands(seed, n, h, w, cin, cout, amp, 1 if nres == 2 else 0)
    kw = dict(slope=EXACT_SLOPE if cout == 32 else None)
    if nres >= 1:
        kw.update(res1=buf[:, :cout], beta1=EXACT_BETA)
    if nres == 2:
        kw.update(res2=res[0][:, R2_OFF:R2_OFF + cout], beta2=EXACT_BETA)
    return buf, wt, bias, (res[0] if nres == 2 else None), kw


# ----------------------------------------------------------------------------- the network
def _store(t, dtype):
    """Storage model: float64 -> fp32 -> the 16-bit type -> float64 (None: no rounding)."""
    if dtype is None:
        return t
    return t.to(torch.float32).to(DTYPES[dtype] if not isinstance(dtype, torch.dtype) else dtype).to(torch.float64)


def _lrelu(v):
    return torch.where(v >= 0, v, v * F32(SLOPE))


def network(sd, x, scale=4, dtype=None, fused=True):
    """RRDBNet forward in float64 from a state_dict (any num_block / num_feat / num_grow_ch: read off the keys) and an fp32
    NCHW input.  dtype=None: pure float64.  Otherwise the storage model of the HIP path: weights, the input and every
    16-bit activation tensor are rounded where that path stores them -- `fused`: as the growth-buffer kernel does (conv5's
    residual steps in fp32, one rounding), else as the composed launches do (x5, each scale-add and the RRDB's own rounded)."""
    st = lambda t: _store(t, dtype)
    wt = lambda k: st(sd[k + ".weight"].double())
    conv = lambda v, k: TF.conv2d(v, wt(k), sd[k + ".bias"].double(), 1, 1)
    beta = F32(BETA)
    u = {4: 1, 2: 2, 1: 4}[scale]
    x = x.double()
    if u > 1:
        x = TF.pixel_unshuffle(x, u)
    feat = st(conv(st(x), "conv_first"))
    nb = 1 + max([int(k.split(".")[1]) for k in sd if k.startswith("body.")], default=-1)
    body = feat
    for i in range(nb):
        x_rrdb = body
        for j in (1, 2, 3):
            p = f"body.{i}.rdb{j}."
            xs = [body]
            for k in range(4):
                xs.append(st(_lrelu(conv(torch.cat(xs, 1), p + f"conv{k + 1}"))))
            x5 = conv(torch.cat(xs, 1), p + "conv5")
            if fused or dtype is None:
                v = x5 * beta + body
                body = st(v * beta + x_rrdb) if j == 3 else st(v)
            else:
                body = st(st(x5) * beta + body)
                if j == 3:
                    body = st(body * beta + x_rrdb)
    feat = st(st(conv(body, "conv_body")) + feat)
    up = lambda v: TF.interpolate(v, scale_factor=2, mode="nearest")
    feat = st(_lrelu(conv(up(feat), "conv_up1")))
    feat = st(_lrelu(conv(up(feat), "conv_up2")))
    feat = st(_lrelu(conv(feat, "conv_hr")))
    return conv(feat, "conv_last")
