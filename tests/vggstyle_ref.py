"""Yardstick of the style (Gram-matrix) term of perceptual.VggFeatureLoss, in float64 torch CPU ops.

Written from the definition, not from the module.  For a tapped map phi of shape [N, C, H, W]
    gram(phi)[n][i][j] = sum_p phi[n][i][p] * phi[n][j][p] / (C H W)                 p over the H W pixels
    style = style_weight * sum_k w_k * crit(gram(phi_k(x1)), gram(phi_k(x2)))
with crit the mean of |.| ('l1') or of (.)^2 ('mse' / 'l2') over the N C C entries, and the layer weights w_k of the content
term.  The trunk is vggfeat_ref.taps (convolutions through the module attribute ``F.conv2d``, so that
``oracle.lowp.storage(torch.bfloat16)`` turns the same code into its 16-bit-storage floor); the Gram matrices, the criterion
and the sum are float64 whatever the trunk's dtype."""
import torch

import vggfeat_ref


def gram(phi):
    n, c, h, w = phi.shape
    m = phi.double().reshape(n, c, h * w)
    return m @ m.transpose(1, 2) / float(c * h * w)


def crit(a, b, criterion):
    if criterion not in ("l1", "mse", "l2"):
        raise ValueError(criterion)
    d = a - b
    return d.abs().mean() if criterion == "l1" else (d * d).mean()


def _taps64(sd, img1, img2, names, use_input_norm, range_norm):
    sd = {k: v.double() for k, v in sd.items()}
    return tuple(vggfeat_ref.taps(sd, vggfeat_ref.preprocess(img.double(), use_input_norm, range_norm), names) for img in (img1, img2))


def ref_style_terms(sd, img1, img2, layer_weights, criterion="l1", use_input_norm=True, range_norm=False):
    """{name: unweighted crit(gram(phi(img1)), gram(phi(img2)))}, float64 scalars"""
    f1, f2 = _taps64(sd, img1, img2, layer_weights, use_input_norm, range_norm)
    return {name: crit(gram(f1[name]), gram(f2[name]), criterion) for name in layer_weights}


def ref_terms(sd, img1, img2, layer_weights, criterion="l1", use_input_norm=True, range_norm=False):
    """({name: content mean}, {name: style mean}) from ONE run of the trunk per image, float64 scalars"""
    f1, f2 = _taps64(sd, img1, img2, layer_weights, use_input_norm, range_norm)
    content = {name: crit(f1[name], f2[name], criterion) for name in layer_weights}
    style = {name: crit(gram(f1[name]), gram(f2[name]), criterion) for name in layer_weights}
    return content, style


def ref_loss(sd, img1, img2, layer_weights, criterion="l1", perceptual_weight=1.0, style_weight=1.0, use_input_norm=True,
             range_norm=False):
    """perceptual_weight * content + style_weight * style; a zero weight drops its half"""
    content, style = ref_terms(sd, img1, img2, layer_weights, criterion, use_input_norm, range_norm)
    total = 0.0
    for name, w in layer_weights.items():
        if perceptual_weight > 0:
            total = total + perceptual_weight * float(w) * content[name]
        if style_weight > 0:
            total = total + style_weight * float(w) * style[name]
    return total
