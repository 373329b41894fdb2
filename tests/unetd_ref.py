"""Float64 CPU yardstick of UNetDiscriminatorSN (models/GAN/unet_discriminator.py) and of the logits GAN loss.

The network is written from BasicSR's published definition (no package and no trained weights were available: parity with
BasicSR is unpinned; tests/test_host_unetd.py holds this file to a copy built from torch.nn.utils.spectral_norm), with an
optional STORAGE MODEL that rounds to the 16-bit type exactly where the HIP path stores a 16-bit tensor: the input image, the
weight images the kernels read (conv0 / conv9 and the eight W_sn), every activation, every upsampled map and every skip
sum.  Biases, the spectral norm itself and the logits stay unrounded (fp32 on the device).  Nothing is imported from the
package under test but _lib's constants (through conv_exact_ref)."""
import math

import torch
import torch.nn.functional as TF

import spectral_ref
from conv_exact_ref import BF16, DTYPES, F16  # noqa: F401

SLOPE = 0.2
SN = tuple(f"conv{i}" for i in range(1, 9))


def layer_table(num_in_ch=3, num_feat=64):
    """[(name, cout, cin, k, stride, normalised)] in forward order."""
    nf = num_feat
    return [("conv0", nf, num_in_ch, 3, 1, False), ("conv1", 2 * nf, nf, 4, 2, True), ("conv2", 4 * nf, 2 * nf, 4, 2, True),
            ("conv3", 8 * nf, 4 * nf, 4, 2, True), ("conv4", 4 * nf, 8 * nf, 3, 1, True), ("conv5", 2 * nf, 4 * nf, 3, 1, True),
            ("conv6", nf, 2 * nf, 3, 1, True), ("conv7", nf, nf, 3, 1, True), ("conv8", nf, nf, 3, 1, True),
            ("conv9", 1, nf, 3, 1, False)]


def key_table(num_in_ch=3, num_feat=64):
    """[(state_dict key, shape)] in torch's order (parameters, then buffers, per child)."""
    out = []
    for name, cout, cin, k, _, sn in layer_table(num_in_ch, num_feat):
        if sn:
            out += [(name + ".weight_orig", (cout, cin, k, k)), (name + ".weight_u", (cout,)), (name + ".weight_v", (cin * k * k,))]
        else:
            out += [(name + ".weight", (cout, cin, k, k)), (name + ".bias", (cout,))]
    return out


def param_count(**kw):
    return sum(math.prod(s) for k, s in key_table(**kw) if not k.endswith(("weight_u", "weight_v")))


def _store(t, dtype):
    if dtype is None:
        return t
    return t.to(torch.float32).to(DTYPES[dtype] if not isinstance(dtype, torch.dtype) else dtype).to(torch.float64)


def network(sd, x, dtype=None, training=True, skip=True):
    """(logits [N, 1, H, W] float64, {layer: (u, v)} as the forward leaves them) from a state_dict and an NCHW input.
    dtype=None: float64 throughout; BF16 / F16: the storage model.  The vectors in `sd` are not modified.  Differentiable
    with respect to float64 leaves in `sd` and `x` (u and v act as constants, as in torch)."""
    st = lambda t: _store(t, dtype)
    # (the published slope, 0.2 in float64: the kernels receive it as fp32, 1.5e-8 away in relative terms)
    lrelu = lambda v: torch.where(v >= 0, v, v * SLOPE)
    up = lambda v: st(TF.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False))
    strides = {name: s for name, _, _, _, s, _ in layer_table()}
    vectors, weights = {}, {}
    for name in SN:
        w, u, v = sd[name + ".weight_orig"].double(), sd[name + ".weight_u"].double(), sd[name + ".weight_v"].double()
        if training:
            with torch.no_grad():
                u, v, _, _ = spectral_ref.iterate(w, u, v)
        sigma = u @ (spectral_ref.mat(w) @ v)              # (differentiable in w; u, v constants)
        weights[name] = st(w / sigma)
        vectors[name] = (u, v)

    def conv(v, name):
        return st(lrelu(TF.conv2d(v, weights[name], None, strides[name], 1)))

    x0 = st(lrelu(TF.conv2d(st(x.double()), st(sd["conv0.weight"].double()), sd["conv0.bias"].double(), 1, 1)))
    x1 = conv(x0, "conv1")
    x2 = conv(x1, "conv2")
    x3 = conv(x2, "conv3")
    add = (lambda a, b: st(a + b)) if skip else (lambda a, b: a)
    x4 = add(conv(up(x3), "conv4"), x2)
    x5 = add(conv(up(x4), "conv5"), x1)
    x6 = add(conv(up(x5), "conv6"), x0)
    out = conv(conv(x6, "conv7"), "conv8")
    return TF.conv2d(out, st(sd["conv9.weight"].double()), sd["conv9.bias"].double(), 1, 1), vectors


def gan_loss(x, target_is_real, kind="vanilla", is_disc=False):
    """BasicSR's GANLoss (unweighted) on logits in the dtype of `x` (float64: the yardstick; float32: the floor), mean over
    all elements, with the formulas of the issue: softplus(z) = max(z, 0) + log1p(exp(-|z|))."""
    if kind == "vanilla":
        z = -x if target_is_real else x
        return (z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))).mean()
    if kind == "lsgan":
        return ((x - (1.0 if target_is_real else 0.0)) ** 2).mean()
    if kind == "hinge":
        if is_disc:
            return torch.relu(1 + (-x if target_is_real else x)).mean()
        return (-x).mean()
    raise ValueError(kind)
