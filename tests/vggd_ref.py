"""Float64 CPU yardstick of BasicSR's VGGStyleDiscriminator, of its dense logit head (flatten -> Linear(K, 100) -> LeakyReLU ->
Linear(100, 1), logits out) and of steps.esrgan_step with that discriminator.  The module itself is not in the package yet
(README, "Not here"); this file is what it will be held to.

The network is written from BasicSR's published definition (no package and no trained weights were available: parity with
BasicSR is unpinned; tests/test_host_vggd.py holds this file to a copy built from torch.nn layers), from torch CPU ops:
conv2d, batch_norm, leaky_relu, linear.  An optional STORAGE MODEL, built the way tests/unetd_ref.py builds one, rounds to the
16-bit type where functional.ConvAct / ConvBNAct store a 16-bit tensor: the input image, the weight images the convolutions
read, conv0_0's activation, and per block the raw convolution output (the batch statistics are taken from the unrounded sums,
as the kernels take them from their fp32 accumulators) and the activation.  With `folded` (eval mode under no_grad) the raw
output is not stored: the affine map rides in the convolution's epilogue.  The BatchNorm parameters and statistics, the dense
head's four parameters and the logits stay unrounded.  Nothing is imported from the package under test but _lib's constants
(through conv_exact_ref)."""
import math

import torch
import torch.nn.functional as TF

import ragan_ref as RG
import rrdb_ref as R
from conv_exact_ref import BF16, DTYPES, F16  # noqa: F401

SLOPE = 0.2
EPS = 1e-5
MOMENTUM = 0.1
HIDDEN = 100
U32 = 2.0 ** -24


def block_table(num_feat=64, input_size=128):
    """[(conv, bn, cout, cin, k, stride)] of the conv + BatchNorm blocks in forward order (conv0_0 comes before them)."""
    nf = num_feat
    widths = [(nf, 2 * nf), (2 * nf, 4 * nf), (4 * nf, 8 * nf), (8 * nf, 8 * nf)] + ([(8 * nf, 8 * nf)] if input_size == 256 else [])
    out = [("conv0_1", "bn0_1", nf, nf, 4, 2)]
    for s, (cin, cout) in enumerate(widths, start=1):
        out += [(f"conv{s}_0", f"bn{s}_0", cout, cin, 3, 1), (f"conv{s}_1", f"bn{s}_1", cout, cout, 4, 2)]
    return out


def key_table(num_in_ch=3, num_feat=64, input_size=128):
    """[(state_dict key, shape)] in torch's order."""
    out = [("conv0_0.weight", (num_feat, num_in_ch, 3, 3)), ("conv0_0.bias", (num_feat,))]
    for conv, bn, cout, cin, k, _ in block_table(num_feat, input_size):
        out += [(conv + ".weight", (cout, cin, k, k)), (bn + ".weight", (cout,)), (bn + ".bias", (cout,)),
                (bn + ".running_mean", (cout,)), (bn + ".running_var", (cout,)), (bn + ".num_batches_tracked", ())]
    out += [("linear1.weight", (HIDDEN, 8 * num_feat * 16)), ("linear1.bias", (HIDDEN,)), ("linear2.weight", (1, HIDDEN)),
            ("linear2.bias", (1,))]
    return out


def param_count(**kw):
    return sum(math.prod(s) for k, s in key_table(**kw) if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))


def _store(t, dtype):
    if dtype is None:
        return t
    return t.to(torch.float32).to(DTYPES[dtype] if not isinstance(dtype, torch.dtype) else dtype).to(torch.float64)


def _lrelu(v):
    return TF.leaky_relu(v, SLOPE)


def network(sd, x, dtype=None, training=True, folded=False, input_size=128, num_feat=None):
    """(logits [N, 1] float64, {key: new value} for every running_mean / running_var / num_batches_tracked) from a state dict and
    an NCHW input.  dtype=None: float64 throughout; BF16 / F16: the storage model.  `sd` is not modified.  Differentiable with
    respect to float64 leaves in `sd` and `x`."""
    st = lambda t: _store(t, dtype)
    nf = sd["conv0_0.weight"].shape[0] if num_feat is None else num_feat
    f = st(_lrelu(TF.conv2d(st(x.double()), st(sd["conv0_0.weight"].double()), sd["conv0_0.bias"].double(), 1, 1)))
    stats = {}
    for conv, bn, _, _, _, stride in block_table(nf, input_size):
        y = TF.conv2d(f, st(sd[conv + ".weight"].double()), None, stride, 1)
        gamma, beta = sd[bn + ".weight"].double(), sd[bn + ".bias"].double()
        rm, rv = sd[bn + ".running_mean"].detach().double().clone(), sd[bn + ".running_var"].detach().double().clone()
        nbt = sd[bn + ".num_batches_tracked"].detach().clone()
        if dtype is None:
            z = TF.batch_norm(y, rm, rv, gamma, beta, training, MOMENTUM, EPS)          # (updates rm and rv in train mode)
        else:
            if training:
                n = y.numel() // y.shape[1]
                mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
                with torch.no_grad():
                    rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
                    rv = (1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)
            else:
                mean, var = rm, rv
            scale = gamma / torch.sqrt(var + EPS)
            shift = beta - mean * scale
            y16 = y if folded else st(y)
            z = y16 * scale[None, :, None, None] + shift[None, :, None, None]
        if training:
            nbt = nbt + 1
        stats[bn + ".running_mean"], stats[bn + ".running_var"], stats[bn + ".num_batches_tracked"] = rm, rv, nbt
        f = st(_lrelu(z))
    h = _lrelu(TF.linear(f.flatten(1), sd["linear1.weight"].double(), sd["linear1.bias"].double()))
    return TF.linear(h, sd["linear2.weight"].double(), sd["linear2.bias"].double()), stats


# ----------------------------------------------------------------------------- the head
def head(x, w1, b1, w2, b2, slope, dout=None, mask_from=None):
    """The dense head in float64 on x [B, K] (C,H,W flatten order): dict of pre, h1, out and -- with dout [B] -- dx, dw1, db1,
    dw2, db2.  The mask is h1 > 0 -> 1, else slope (torch's rule at 0), read off `mask_from` when given (the device's h1)."""
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    pre = x @ w1.t() + b1
    h1 = torch.where(pre >= 0, pre, pre * slope)
    out = h1 @ w2.reshape(-1) + b2.reshape(())
    res = dict(pre=pre, h1=h1, out=out)
    if dout is not None:
        dout = dout.double().reshape(-1)
        one = torch.ones((), dtype=torch.float64)
        m = torch.where((h1 if mask_from is None else mask_from.double()) > 0, one, one * float(slope))
        dh = dout[:, None] * w2.reshape(1, -1) * m
        res.update(dh=dh, dx=dh @ w1, dw1=dh.t() @ x, db1=dh.sum(0), dw2=(dout[:, None] * h1).sum(0).reshape(1, -1),
                   db2=dout.sum().reshape(1))
    return res


def head_bounds(x, w1, b1, w2, b2, h1):
    """(bound of h1 [B, O], bound of out [B]) for fp32 fmaf chains of any fixed order: a sum of n terms carries at most
    n 2^-24 sum|terms| (first order), and no chain of a head over K columns and O hidden units -- however k is cut into slices,
    with the bias, the slope, the second layer, its bias and the rounding of the reference -- is longer than K + O + 4.  The
    first layer's bound reaches the logit through |w2|."""
    x, w1, b1, w2, b2, h1 = (t.double() for t in (x, w1, b1, w2, b2, h1))
    k, o = x.shape[1], w1.shape[0]
    n = (k + o + 4) * U32
    bh = n * (x.abs() @ w1.abs().t() + b1.abs())
    bo = bh @ w2.abs().reshape(-1) + n * ((h1 * w2.reshape(1, -1)).abs().sum(1) + b2.abs().reshape(()))
    return bh, bo


def nhwc(x_flat, c, cp, hw, dtype, pad_bits=None):
    """[B, K] float64 in C,H,W flatten order -> the 16-bit NHWC map [B, HW, Cp] of functional.py; the pad channels are zero, or the
    given 16-bit pattern (garbage a kernel must never read)."""
    b = x_flat.shape[0]
    t16 = DTYPES[dtype]
    out = torch.zeros((b, hw, cp), dtype=t16)
    if pad_bits is not None:
        out.view(torch.int16)[:] = pad_bits
    out[:, :, :c] = x_flat.reshape(b, c, hw).permute(0, 2, 1).to(torch.float32).to(t16)
    return out


def from_nhwc(t, c):
    """[B, HW, Cp] -> [B, K] float64 in C,H,W flatten order."""
    return t[:, :, :c].double().permute(0, 2, 1).reshape(t.shape[0], -1)


# ----------------------------------------------------------------------------- the step
def step_reference(gsd, dsd, lq, gt, dtype, l1_weight, gan_weight, gan_type="vanilla"):
    """steps.esrgan_step with VGGStyleDiscriminator and no content term, restated on tests/ragan_ref.py's loss: float64
    (dtype=None) or the storage model.  Returns the five losses (with their 1/2 inside), the generator's gradients and D's state
    after its five train-mode forwards (weights untouched: the optimiser's step is not restated)."""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in gsd.items()}
    gt64 = gt.double()
    fake = R.network(leaves, lq, 4, dtype=dtype, fused=False)
    l_pix = (fake - gt64).abs().mean()
    d = {k: (v.double() if v.is_floating_point() else v).clone() for k, v in dsd.items()}
    size = gt.shape[-1]

    def disc(img):
        y, stats = network(d, img, dtype, True, False, size)
        d.update(stats)
        return y

    rel = lambda x, o, real, is_disc: RG.rel_gan_loss(x, o, real, gan_type, is_disc)
    with torch.no_grad():
        real_pred = disc(gt64)
    fake_pred = disc(fake)
    l_g_gan = 0.5 * (rel(real_pred, fake_pred, False, False) + rel(fake_pred, real_pred, True, False))
    (l1_weight * l_pix + gan_weight * l_g_gan).backward()
    grads = {k: v.grad for k, v in leaves.items()}
    with torch.no_grad():
        fake_pred = disc(fake.detach())
        real_pred = disc(gt64)
        l_d_real = 0.5 * rel(real_pred, fake_pred, True, True)
        fake_pred = disc(fake.detach())
        l_d_fake = 0.5 * rel(fake_pred, real_pred, False, True)
    losses = [float(v.detach()) for v in (l_pix, 0.0 * l_pix, l_g_gan, l_d_real, l_d_fake)]
    return losses, grads, d
