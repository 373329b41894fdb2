"""Generator inference (eval_GAN.py:44,94: ``gan_G.eval()`` then ``gan_G(LR_image)``), whole-image or tiled.

In eval mode every BatchNorm is a fixed affine map, so the generator is a pure convolution stack with a finite
receptive field: 4 (9x9 head) + 2*blocks + 1 (3x3 trunk) LR pixels, plus 1, 1/2, 1/4 ... for the shuffle convs and
4/factor for the 9x9 tail -- 40 LR pixels for the 16-block x8 model.  A tile computed with that much
halo is therefore bit-identical to the same region of the whole-image result; tiling only bounds the activation
footprint (64 channels at 8x resolution) when images are large.  BASELINE config 5 runs this in fp16.
A model that carries ``scale`` and ``receptive_halo()`` itself (models/GAN/rrdbnet.py) is tiled by those; one that starts with
``pixel_unshuffle`` (its ``unshuffle`` factor) needs ``tile`` and ``halo`` to be multiples of that factor.

Geometric self-ensemble (EDSR "+", Lim et al. 2017): the generator runs on the eight flipped / turned copies of the LR
image, each output is turned back and the eight are averaged.  The copies and the inverse-and-mean are one HIP launch
each (csrc/d4.hip); ``d4`` / ``d4_inverse`` are the transform itself.  Code k in 0..7: k % 4 quarter turns, of the
left-right mirrored image when k >= 4 -- ``torch.rot90(torch.flip(x, [-1]) if k >= 4 else x, k % 4, [-2, -1])``.
"""
import torch

from . import _lib
from .functional import _ptr, _stream


def receptive_halo(gen):
    own = getattr(gen, "receptive_halo", None)
    if callable(own):                        # a model that knows its own receptive field (models/GAN/rrdbnet.py)
        return own()
    blocks = len(gen.residual_blocks)
    return 4 + 2 * blocks + 1 + 2 + 1        # head + trunk + conv2 + shuffle convs/tail (rounded up)


def _factor(gen):
    scale = getattr(gen, "scale", None)
    return int(scale) if scale is not None else 2 ** len(gen.pixel_shuffle_blocks)


def _check_image(x, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise TypeError(f"{what}: a float32 NCHW tensor on the device is expected")
    return x.contiguous()


def _check_code(k):
    k = int(k)
    if not 0 <= k <= 7:
        raise ValueError(f"transform code {k} is not in 0..7")
    return k


def d4(x, k):
    """T_k of an fp32 NCHW device tensor: [N,C,H,W] for even k, [N,C,W,H] for odd k (dsr_d4_expand_f32, one code)."""
    k = _check_code(k)
    x = _check_image(x, "d4")
    n, c, h, w = x.shape
    out = torch.empty((n, c, w, h) if k % 2 else (n, c, h, w), dtype=torch.float32, device=x.device)
    even, odd = (None, _ptr(out)) if k % 2 else (_ptr(out), None)
    _lib.check(_lib.lib().dsr_d4_expand_f32(_ptr(x), n * c, h, w, 1 << k, even, odd, _stream()))
    return out


def d4_inverse(y, k):
    """T_k^-1: ``d4_inverse(d4(x, k), k)`` is x.  A quarter turn is undone by the opposite one (1 <-> 3); the mirrored codes
    are reflections, each its own inverse."""
    k = _check_code(k)
    return d4(y, k if k >= 4 else (4 - k) % 4)


def _run(gen, lr, tile, halo):
    if tile is None:
        return gen(lr)
    n, _, h, w = lr.shape
    halo = receptive_halo(gen) if halo is None else halo
    f = _factor(gen)
    u = int(getattr(gen, "unshuffle", 1))
    if u > 1 and (tile % u or halo % u):
        # a model that starts with pixel_unshuffle: every tile must start on its grid
        raise ValueError(f"super_resolve: tile ({tile}) and halo ({halo}) must be multiples of the model's pixel_unshuffle factor {u}")
    out = torch.empty((n, 3, h * f, w * f), dtype=torch.float32, device=lr.device)
    for y0 in range(0, h, tile):
        for x0 in range(0, w, tile):
            y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
            ya, xa = max(y0 - halo, 0), max(x0 - halo, 0)
            yb, xb = min(y1 + halo, h), min(x1 + halo, w)
            sr = gen(lr[:, :, ya:yb, xa:xb].contiguous())
            out[:, :, y0 * f:y1 * f, x0 * f:x1 * f] = sr[:, :, (y0 - ya) * f:(y1 - ya) * f, (x0 - xa) * f:(x1 - xa) * f]
    return out


def _run_copies(gen, copies, tile, halo, ensemble_batch):
    """The generator on a batch of transformed copies, `ensemble_batch` at a time (None: all at once)."""
    n = copies.shape[0]
    if ensemble_batch is None or ensemble_batch >= n:
        return _run(gen, copies, tile, halo)
    out = None
    for i in range(0, n, ensemble_batch):
        sr = _run(gen, copies[i:i + ensemble_batch], tile, halo)
        if out is None:
            out = torch.empty((n,) + tuple(sr.shape[1:]), dtype=torch.float32, device=sr.device)
        out[i:i + ensemble_batch] = sr
    return out


def _self_ensemble(gen, lr, codes, tile, halo, ensemble_batch):
    lib = _lib.lib()
    lr = _check_image(lr, "super_resolve")
    mask = 0
    for k in codes:
        mask |= 1 << k
    n_even, n_odd = bin(mask & 0x55).count("1"), bin(mask & 0xAA).count("1")
    n, c, h, w = lr.shape
    dev, st = lr.device, _stream()
    result = None
    for b in range(n):
        # the copies: [n_even,c,h,w] and [n_odd,c,w,h]; for a square image one [n_even + n_odd,c,h,h] batch holds both
        if h == w:
            both = torch.empty((n_even + n_odd, c, h, w), dtype=torch.float32, device=dev)
            even, odd = both[:n_even], both[n_even:]
        else:
            both = None
            even = torch.empty((n_even, c, h, w), dtype=torch.float32, device=dev)
            odd = torch.empty((n_odd, c, w, h), dtype=torch.float32, device=dev)
        _lib.check(lib.dsr_d4_expand_f32(_ptr(lr[b]), c, h, w, mask, _ptr(even) if n_even else None, _ptr(odd) if n_odd else None, st))
        if both is not None:
            sr = _run_copies(gen, both, tile, halo, ensemble_batch)
            sr_even, sr_odd = sr[:n_even], sr[n_even:]
        else:
            sr_even = _run_copies(gen, even, tile, halo, ensemble_batch) if n_even else None
            sr_odd = _run_copies(gen, odd, tile, halo, ensemble_batch) if n_odd else None
        some = sr_even if n_even else sr_odd
        co = some.shape[1]
        H, W = (some.shape[2], some.shape[3]) if n_even else (some.shape[3], some.shape[2])
        if result is None:
            result = torch.empty((n, co, H, W), dtype=torch.float32, device=dev)
        _lib.check(lib.dsr_d4_mean_f32(_ptr(sr_even) if n_even else None, _ptr(sr_odd) if n_odd else None, co, H, W, mask,
                                       _ptr(result[b]), st))
    return result


@torch.no_grad()
def super_resolve(gen, lr, tile=None, halo=None, dtype=torch.float16, self_ensemble=False, ensemble_batch=None):
    """lr: fp32 NCHW [N,3,h,w] on the GPU -> fp32 [N,3,h*f,w*f].  tile=None runs the whole image at once.

    self_ensemble: True = the mean over all eight D4 copies of the image, or a sequence of codes (e.g. ``(0, 4)``: the
    image and its mirror).  Per image: one launch writes the copies, the generator runs on them, one launch turns the
    outputs back and averages them in fp32, in ascending code order.  ensemble_batch=None runs all copies of one shape as
    one batch (eight at once for a square image, four and four otherwise); ensemble_batch=b runs b copies per generator
    call -- with 1 every copy gets the launches a plain ``super_resolve`` of it would.  With ``tile=`` every copy goes
    through the tiled path.  A batch whose activations exceed the conv kernels' 2 GiB tensor limit is refused by them
    (eight copies at 256 x 256 -> 2048 x 2048 are): give ``ensemble_batch`` there."""
    codes = None
    if self_ensemble is True:
        codes = list(range(8))
    elif self_ensemble is not False and self_ensemble is not None:
        codes = sorted({_check_code(k) for k in self_ensemble})
        if not codes:
            raise ValueError("self_ensemble: an empty set of codes")
    if ensemble_batch is not None and int(ensemble_batch) < 1:
        raise ValueError("ensemble_batch must be a positive number of copies or None")
    was_training = gen.training
    old = gen.compute_dtype
    gen.eval()
    gen.compute_dtype = dtype
    try:
        if codes is None:
            return _run(gen, lr, tile, halo)
        return _self_ensemble(gen, lr, codes, tile, halo, None if ensemble_batch is None else int(ensemble_batch))
    finally:
        gen.compute_dtype = old
        gen.train(was_training)
