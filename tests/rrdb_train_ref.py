"""Float64 CPU yardstick of the backward of a dense block on its growth buffers (csrc/conv_rdb.hip's input-gradient form,
csrc/conv_rdb_bwd.hip, functional.RRDBBody), on top of tests/rrdb_ref.py.

B is a block's forward buffer [N, 192, H, W] here (x in [0, 64), x_k in [64 + 32 (k - 1), 64 + 32 k)), G a gradient buffer of
the same shape.  The five input-gradient launches of a block, k = 5 .. 1:
    k = 5     G[0:192]  = scale * dgrad5(g);  channels [0, 64) += g_scale * g;  channels [160, 192) times the mask of x_4
    k = 4..2  G[0:c]   += dgrad_k(G[c:c + 32]),  c = 64 + 32 (k - 1);  channels [c - 32, c) times the mask of x_(k-1)
    k = 1     G[0:64]  += dgrad_1(G[64:96])  (+ the dL/dout of the RRDB for its first block)
mask = 1 where the stored activation is >= 0, else slope.  Nothing is imported from the package under test."""
import torch
import torch.nn.functional as TF

import rrdb_ref as R
from rrdb_ref import small_ints, ternary

F, G, LD = 64, 32, 192
EXACT_SLOPE = EXACT_BETA = 0.25
DGRAD_SHAPES = [(1, 9, 65), (2, 12, 20), (1, 17, 130), (2, 1, 1)]     # (N, H, W): the pixel tile is 8 x 64


def launch_geometry(k):
    """(K, dy_off, Cout, mask_lo or None) of dgrad_k."""
    if k == 5:
        return 64, 0, 192, 160
    c = F + G * (k - 1)
    return 32, c, c, (c - 32 if k > 1 else None)


def dgrad_value(dy, weight, old, scale=1.0, g=None, g_scale=1.0, act=None, mask_lo=None, slope=None):
    """Unrounded float64 value of one launch over channels [0, Cout): dy [N, K, H, W], weight [K, Cout, 3, 3] (the forward
    convolution's OIHW weight), old [N, Cout, H, W] or None (the accumulate), g [N, 64, H, W] or None, act [N, Cout, H, W]."""
    v = TF.conv_transpose2d(dy.double(), weight.double(), None, 1, 1) * scale
    if old is not None:
        v = v + old.double()
    if g is not None:
        v = torch.cat([v[:, :F] + g.double() * g_scale, v[:, F:]], 1)
    if mask_lo is not None:
        m = torch.where(act.double()[:, mask_lo:] >= 0, 1.0, float(slope))
        v = torch.cat([v[:, :mask_lo], v[:, mask_lo:] * m], 1)
    return v


def dgrad_bound(dy, weight, old, scale=1.0, g=None, g_scale=1.0):
    """A of |v - v64| <= u |v64| + (9 K + 4) 2^-24 A: the same sum with absolute values (the mask is at most 1)."""
    a = TF.conv_transpose2d(dy.double().abs(), weight.double().abs(), None, 1, 1) * abs(scale)
    if old is not None:
        a = a + old.double().abs()
    if g is not None:
        a = torch.cat([a[:, :F] + g.double().abs() * abs(g_scale), a[:, F:]], 1)
    return a


def exact_dgrad_case(n, h, w, k, amp=3):
    """Integer operands of launch k: (B, G before, g or None, weight, keyword arguments of dgrad_value without `old`).
    B and G in [-amp, amp] on all 192 channels, ternary weights of density 0.25, slope 0.25; k = 5 takes a dense g with
    scale = g_scale = 0.25 (the third block's form: both factors differ from 1), k = 1 the RRDB's g with g_scale = 1."""
    gen = torch.Generator().manual_seed(7000 + 1000 * n + 100 * h + 10 * w + k + amp)
    K, dy_off, cout, mask_lo = launch_geometry(k)
    B = small_ints(gen, (n, LD, h, w), amp)
    G0 = small_ints(gen, (n, LD, h, w), amp)
    wt = ternary(gen, (K, cout, 3, 3), 0.25)
    g = small_ints(gen, (n, F, h, w), amp) if k in (5, 1) else None
    kw = dict(scale=EXACT_BETA if k == 5 else 1.0, g=g, g_scale=EXACT_BETA if k == 5 else 1.0, mask_lo=mask_lo,
              slope=EXACT_SLOPE)
    return B, G0, g, wt, kw


def block_param_grads(B, Gm, g, gscale):
    """Float64 weight and bias gradients of the five convolutions of one block: B [N, 192, H, W], Gm [N, 192, H, W] whose
    channels [64, 192) hold dY_1..4, g [N, 64, H, W], dY_5 = gscale * g.  Returns ([dW_1..5], [db_1..5])."""
    B, Gm, g = B.double(), Gm.double(), g.double()
    dws, dbs = [], []
    for k in range(5):
        cin = F + G * k
        dy = Gm[:, cin:cin + G] if k < 4 else g * gscale
        dws.append(torch.nn.grad.conv2d_weight(B[:, :cin], (dy.shape[1], cin, 3, 3), dy, stride=1, padding=1))
        dbs.append(dy.sum((0, 2, 3)))
    return dws, dbs


def exact_wgrad_case(n, h, w, amp=3):
    gen = torch.Generator().manual_seed(9000 + 1000 * n + 100 * h + w)
    return small_ints(gen, (n, LD, h, w), amp), small_ints(gen, (n, LD, h, w), amp), small_ints(gen, (n, F, h, w), amp)


def wgrad_tiles(n, h, w):
    """Tiles of the weight-gradient kernel (2 rows x 32 columns of one image)."""
    return n * ((h + 1) // 2) * ((w + 31) // 32)


# ----------------------------------------------------------------------------- the launchers' work partition, restated
RDB_GRID_CAP = R.RDB_GRID_CAP   # csrc/conv_rdb.hip: blocks of a forward / input-gradient launch unless max_blocks overrides it
WGRAD_WANT, COLSUM_ROWS, COLSUM_MIN_PPB = 64, 256, 64          # csrc/conv_rdb_bwd.hip, rdb_wgrad_plan


def dgrad_slices(k):
    """Output-channel slices per tile of dgrad_k: Cout / 64 where 64 divides Cout, else Cout / 32."""
    cout = launch_geometry(k)[2]
    return cout // 64 if cout % 64 == 0 else cout // 32


def dgrad_plan(n, h, w, k, max_blocks=0):
    """(work items, blocks) of dgrad_k: item t is slice t % nslices of tile t / nslices, block b walks b, b + blocks, ..."""
    items = R.rdb_tiles(n, h, w) * dgrad_slices(k)
    return items, min(items, max_blocks if max_blocks > 0 else RDB_GRID_CAP)


def dgrad_walk(n, h, w, k, max_blocks=0):
    """[[(image, tile of the image, slice), ...] per block]: the items of each block in the order it takes them."""
    per_img, ns = R.rdb_tiles(1, h, w), dgrad_slices(k)
    items, blocks = dgrad_plan(n, h, w, k, max_blocks)
    return [[((t // ns) // per_img, (t // ns) % per_img, t % ns) for t in range(b, items, blocks)] for b in range(blocks)]


# (N, H, W, k, max_blocks) of the forced partitions: 8 ragged tiles over two images with one block, three blocks and one
# block per slice; 9 tiles with an interior column boundary on two blocks
DGRAD_FORCED = [(2, 9, 65, k, mb) for k in (1, 2, 3, 4, 5) for mb in sorted({1, 3, dgrad_slices(k)})] + \
               [(1, 17, 130, k, 2) for k in (1, 2, 3, 4, 5)]
DGRAD_CAP_SHAPE = (65, 9, 65)          # 260 tiles: every k has more than RDB_GRID_CAP items without max_blocks
DGRAD_FLOAT_PARTITIONS = (0, 1, 3, 5)  # max_blocks of the partition-independence test on float data, (2, 9, 65), k = 2, 4, 5
WGRAD_SCALED_SHAPE = (2, 174, 65)      # 522 tiles, 22,620 pixels: tiles_per_block 9, 58 chunks, cs_ppb 89, 255 column-sum rows


def wgrad_plan(n, h, w):
    """rdb_wgrad_plan of csrc/conv_rdb_bwd.hip: tiles, tiles per chunk, chunks, column-sum pixels per block and rows, bytes."""
    tiles = wgrad_tiles(n, h, w)
    tpb = max(8, -(-tiles // WGRAD_WANT))
    chunks = -(-tiles // tpb)
    pix = n * h * w
    ppb = max(COLSUM_MIN_PPB, -(-pix // COLSUM_ROWS))
    rows = -(-pix // ppb)
    nbytes = 4 * (chunks * 9 * (128 + 64) * LD + rows * LD)
    return dict(tiles=tiles, tiles_per_block=tpb, chunks=chunks, cs_ppb=ppb, cs_rows=rows, bytes=nbytes)


def network_grads(sd, x, probe, dtype, scale=4):
    """Gradients of sum(network(x) * probe) for every state_dict entry and the input ('input'): float64 (dtype=None) or
    the storage model with the fused rounding points (rrdb_ref.network(..., dtype, fused=True))."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xi = x.double().clone().requires_grad_(True)
    y = R.network(leaves, xi, scale, dtype=dtype, fused=True)
    (y * probe.double()).sum().backward()
    out = {k: v.grad for k, v in leaves.items()}
    out["input"] = xi.grad
    return out
