"""Yardstick of perceptual.VggFeatureLoss: the multi-layer VGG19 feature loss restated in plain fp32 torch.

Written from the definition, not from the module:  loss = sum_k w_k * mean_crit(phi_k(x1), phi_k(x2)), phi_k the output of a
VGG19 convolution before ('conv{b}_{i}') or after ('relu{b}_{i}') its ReLU; blocks of 2, 2, 4, 4, 4 convolutions with a 2x2
max-pool behind blocks 1 .. 4.  `sd` holds torchvision's ``vgg19().features`` keys ('<index>.weight', '<index>.bias').
Convolutions go through the module attribute ``F.conv2d`` so that ``oracle.lowp.storage(torch.bfloat16)`` turns the same code
into its 16-bit-storage floor."""
import torch
import torch.nn.functional as F

BLOCKS = (2, 2, 4, 4, 4)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def layer_table():
    """name -> (index of the convolution in torchvision's features Sequential, tapped after the ReLU?)"""
    table = {}
    idx = 0
    for b, n in enumerate(BLOCKS, start=1):
        for i in range(1, n + 1):
            table[f"conv{b}_{i}"] = (idx, False)
            table[f"relu{b}_{i}"] = (idx, True)
            idx += 2                      # conv, relu
        idx += 1                          # the max-pool behind the block
    return table


def preprocess(img, use_input_norm=True, range_norm=False, resize=None, crop=None):
    x = img
    if range_norm:
        x = (x + 1.0) / 2.0
    if resize is not None:
        n, c, h, w = x.shape
        nh, nw = (resize, int(resize * w / h)) if h <= w else (int(resize * h / w), resize)
        x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)
        top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
        x = x[:, :, top:top + crop, left:left + crop]
    if use_input_norm:
        mean = torch.tensor(MEAN, dtype=x.dtype)[None, :, None, None]
        std = torch.tensor(STD, dtype=x.dtype)[None, :, None, None]
        x = (x - mean) / std
    return x


def taps(sd, x, names):
    """{name: feature map} for the requested layers of the trunk applied to the preprocessed batch x."""
    table = layer_table()
    want = {}
    for name in names:
        if name not in table:
            raise ValueError(f"unknown layer {name!r}")
        want.setdefault(table[name], name)
    deepest = max(i for i, _ in want)
    out = {}
    idx = 0
    for b, n in enumerate(BLOCKS, start=1):
        for _ in range(n):
            x = F.conv2d(x, sd[f"{idx}.weight"], sd[f"{idx}.bias"], padding=1)
            if (idx, False) in want:
                out[want[(idx, False)]] = x
            x = F.relu(x)
            if (idx, True) in want:
                out[want[(idx, True)]] = x
            if idx == deepest:
                return out
            idx += 2
        x = F.max_pool2d(x, 2, 2)
        idx += 1
    return out


def ref_terms(sd, img1, img2, layer_weights, criterion="l1", use_input_norm=True, range_norm=False, resize=None, crop=None):
    """{name: unweighted mean |phi(img1) - phi(img2)| (criterion 'l1') or mean (..)^2 ('mse' / 'l2')}"""
    if criterion not in ("l1", "mse", "l2"):
        raise ValueError(criterion)
    f1 = taps(sd, preprocess(img1, use_input_norm, range_norm, resize, crop), layer_weights)
    f2 = taps(sd, preprocess(img2, use_input_norm, range_norm, resize, crop), layer_weights)
    terms = {}
    for name in layer_weights:
        d = f1[name] - f2[name]
        terms[name] = d.abs().mean() if criterion == "l1" else (d * d).mean()
    return terms


def ref_loss(sd, img1, img2, layer_weights, criterion="l1", use_input_norm=True, range_norm=False, resize=None, crop=None):
    terms = ref_terms(sd, img1, img2, layer_weights, criterion, use_input_norm, range_norm, resize, crop)
    total = 0.0
    for name, w in layer_weights.items():
        total = total + float(w) * terms[name]
    return total
