"""Multi-layer VGG19 feature loss on the HIP path: the content term of SRGAN / ESRGAN / Real-ESRGAN, and the style
(Gram-matrix) term of EnhanceNet / SRFeat and of basicsr's ``style_weight``.

utils.GAN.Vgg19Loss is the reference's choice: one tap (relu5_4, after the activation), MSE, behind torchvision's
resize-256 / crop-224 preset.  The published recipes use something else:
  SRGAN paper, ESRGAN   conv5_4 BEFORE the activation
  Real-ESRGAN and later five taps conv1_2 .. conv5_4 with weights 0.1, 0.1, 1, 1, 1, compared by L1, on the image at its own size
VggFeatureLoss expresses both (the constructor follows basicsr's PerceptualLoss, restated from its documented behaviour; parity
with basicsr itself is not pinned by a test, for the content term or the style term).  Each tap is ONE pass over the 16-bit NHWC
map where it already lives (functional.FeatureTap, csrc/featloss.hip): no fp32 NCHW copy of a map, and the Handover chain that
removed the trunk's activation-backward passes stays intact on every untapped layer.  With style_weight > 0 a tap also forms
the map's Gram matrices by MFMA over the same 16-bit map and its backward is still one launch with one rounding per element
(functional.FeatureStyleTap, csrc/featstyle.hip).
"""
import ctypes as C
import math
import re

import numpy as np
import torch
import torch.nn as nn

from . import functional as F
from .utils import GAN as _G

VGG19_BLOCKS = (2, 2, 4, 4, 4)                  # convolutions per block; a 2x2 max-pool follows blocks 1 .. 4
_POOL_AFTER = {sum(VGG19_BLOCKS[:b + 1]) - 1 for b in range(4)}      # conv ordinals 1, 3, 7, 11
_NAME = re.compile(r"^(conv|relu)([1-5])_([1-4])$")


def parse_layer(name):
    """'conv{b}_{i}' (before the activation) / 'relu{b}_{i}' (after it) -> (conv ordinal 0 .. 15, is_post_activation)."""
    m = _NAME.match(name) if isinstance(name, str) else None
    if m is None or int(m.group(3)) > VGG19_BLOCKS[int(m.group(2)) - 1]:
        raise ValueError(f"VggFeatureLoss: unknown layer {name!r} (conv{{b}}_{{i}} or relu{{b}}_{{i}}, b = 1..5, "
                         f"i = 1..{VGG19_BLOCKS} convolutions per block)")
    b, i = int(m.group(2)), int(m.group(3))
    return sum(VGG19_BLOCKS[:b - 1]) + i - 1, m.group(1) == "relu"


class _IdentityTables:
    """The tables functional.ResizeNorm reads, for NO resampling: every output pixel is its input pixel (one weight of 1), so
    the pass is the per-channel affine map (x - mean) / std into 16-bit NHWC."""

    def __init__(self, h, w, device, mean, std):
        wy = [(i, np.ones(1, dtype=np.float32)) for i in range(h)]
        wx = [(i, np.ones(1, dtype=np.float32)) for i in range(w)]
        self.kt = 1
        self.in_h, self.in_w, self.out_h, self.out_w = h, w, h, w

        def dev(arrs):
            return [torch.from_numpy(a).to(device) for a in arrs]

        self.ys, self.yc, self.yw = dev(_G._pack_tables(wy, 1))
        self.xs, self.xc, self.xw = dev(_G._pack_tables(wx, 1))
        self.tys, self.tyc, self.tyw = dev(_G._pack_tables(_G._transpose_windows(wy, h), 1))
        self.txs, self.txc, self.txw = dev(_G._pack_tables(_G._transpose_windows(wx, w), 1))
        self.mean_c = (C.c_float * 3)(*mean)
        self.std_c = (C.c_float * 3)(*std)


class VggFeatureLoss(nn.Module):
    """loss = perceptual_weight * sum_k w_k * mean_crit(phi_k(image1), phi_k(image2))
            + style_weight * sum_k w_k * mean_crit(gram(phi_k(image1)), gram(phi_k(image2)))
    over taps phi_k of a frozen VGG19 trunk; gram(phi)[n][i][j] = sum_p phi[n][i][p] phi[n][j][p] / (C H W) over the H W pixels.

    layer_weights   {name: weight}; 'conv{b}_{i}' taps the map BEFORE the activation, 'relu{b}_{i}' after it (b = 1..5, i over
                    the block's 2, 2, 4, 4, 4 convolutions).  Weights are finite and >= 0, at least one > 0.
    criterion       'l1' or 'mse' ('l2' is an alias of 'mse'); the mean runs over all N C H W elements of a map, and over the
                    N C C entries of its Gram matrices in the style term.  basicsr's 'fro' is not offered (ValueError).
    perceptual_weight, style_weight   finite and >= 0, at least one > 0.  style_weight = 0.0 (default): the content term alone,
                    the launches and the bits of a module built without the keyword.  perceptual_weight = 0: the style term
                    alone, and no content launch runs.  The style term needs C <= 512 (every VGG19 layer).
    use_input_norm  apply the ImageNet mean / std; range_norm maps [-1, 1] -> [0, 1] first.  Both fold into one affine map per
                    channel inside the pass that makes the 16-bit NHWC input.
    state_dict      a torchvision ``vgg19().features`` state dict (keys '<i>.weight' / '<i>.bias'); None: the deterministic
                    stand-ins of utils.GAN.  The module's own keys are Vgg19Loss's, ``net.0.<i>.*``.  The trunk is frozen and
                    runs only as far as the deepest requested tap.
    resize_to, crop both None (default): no resampling, the trunk sees the image at its own size, and a size whose map is odd in
                    front of a max-pool that runs raises ValueError before any launch.  Both given: torchvision's
                    resize / centre-crop preset exactly as in Vgg19Loss (odd maps are floored by the pools, as there).
    compute_dtype   torch.bfloat16 (default, the tested path) or torch.float16.  fp16 goes through the same kernels with NO
                    internal gradient scale: the caller's loss scale (optim.DynamicLossScaler) has to cover it.

    forward(image1, image2, features2=None, grams2=None) returns ONE scalar, content + style, so every caller of a content
    loss (steps.gen_perceptual_step, steps.realesrgan_step, steps.gan_step, utils.GAN.PerceptualLoss(vgg_loss=...)) takes a
    style-weighted module as it is; the content term those report then includes the style term.  It gives a gradient for
    image1 ONLY: an image2 that requires grad raises ValueError (detach it).  terms(...) takes the same arguments and returns
    the two halves (percep, style) as basicsr's forward does, None for a zero weight.  target_features(image) runs under
    no_grad and returns the tuple of 16-bit taps that ``features2=`` accepts, target_grams(features2) the tuple of their fp32
    [N, C, C] Gram matrices that ``grams2=`` accepts, so a step can compute the target's half ahead of time on another stream
    (steps.gan_step does).  After a call ``last_terms`` / ``last_style_terms`` hold the unweighted per-tap means of the two
    halves, {name: 1-element device tensor} (empty for a zero weight); nothing is read on the host."""

    def __init__(self, layer_weights=None, criterion='l1', perceptual_weight=1.0, use_input_norm=True, range_norm=False,
                 state_dict=None, resize_to=None, crop=None, compute_dtype=torch.bfloat16, style_weight=0.0):
        super().__init__()
        layer_weights = {'conv5_4': 1.0} if layer_weights is None else dict(layer_weights)
        if not layer_weights:
            raise ValueError("VggFeatureLoss: layer_weights is empty")
        taps = []
        for name, w in layer_weights.items():
            ordinal, post = parse_layer(name)
            try:
                w = float(w)
            except (TypeError, ValueError):
                raise ValueError(f"VggFeatureLoss: weight of {name!r} is not a number: {w!r}")
            if not math.isfinite(w) or w < 0.0:
                raise ValueError(f"VggFeatureLoss: weight of {name!r} must be finite and >= 0, got {w!r}")
            taps.append((ordinal, post, name, w))
        if not any(w > 0.0 for _, _, _, w in taps):
            raise ValueError("VggFeatureLoss: at least one layer weight must be > 0")
        crit = {'l1': F.FEAT_L1, 'mse': F.FEAT_MSE, 'l2': F.FEAT_MSE}.get(criterion if isinstance(criterion, str) else None)
        if crit is None:
            raise ValueError(f"VggFeatureLoss: criterion {criterion!r} is not 'l1', 'mse' or 'l2'")
        pw = float(perceptual_weight)
        if not math.isfinite(pw) or pw < 0.0:
            raise ValueError(f"VggFeatureLoss: perceptual_weight must be finite and >= 0, got {perceptual_weight!r}")
        try:
            sw = float(style_weight)
        except (TypeError, ValueError):
            raise ValueError(f"VggFeatureLoss: style_weight is not a number: {style_weight!r}")
        if not math.isfinite(sw) or sw < 0.0:
            raise ValueError(f"VggFeatureLoss: style_weight must be finite and >= 0, got {style_weight!r}")
        if pw == 0.0 and sw == 0.0:
            raise ValueError("VggFeatureLoss: perceptual_weight and style_weight are both 0; at least one must be > 0")
        if (resize_to is None) != (crop is None):
            raise ValueError("VggFeatureLoss: give both resize_to and crop (the preset) or neither (no resampling)")
        if compute_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"VggFeatureLoss: compute_dtype must be bfloat16 or float16, got {compute_dtype}")
        taps.sort(key=lambda e: (e[0], e[1]))                     # trunk order; a layer's conv tap comes before its relu tap
        self.taps = tuple(taps)
        self.layer_names = tuple(name for _, _, name, _ in taps)
        self.mode, self.criterion, self.perceptual_weight, self.style_weight = crit, criterion, pw, sw
        self.depth = taps[-1][0] + 1                              # convolutions that run
        layers = []
        cin = 3
        for v in _G.VGG19_CFG:                                    # the trunk Vgg19Loss builds: same keys net.0.<i>.*
            if v == 'M':
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.net = nn.Sequential(nn.Sequential(*layers))
        self.net[0].load_state_dict(state_dict if state_dict is not None else _G._standin_vgg_state())
        self.pretrained = state_dict is not None
        for param in self.net.parameters():
            param.requires_grad = False
        self.use_input_norm, self.range_norm = bool(use_input_norm), bool(range_norm)
        mean = _G.IMAGENET_MEAN if self.use_input_norm else (0.0, 0.0, 0.0)
        std = _G.IMAGENET_STD if self.use_input_norm else (1.0, 1.0, 1.0)
        if self.range_norm:                                       # ((x + 1) / 2 - m) / s = (x - (2 m - 1)) / (2 s)
            mean, std = tuple(2.0 * m - 1.0 for m in mean), tuple(2.0 * s for s in std)
        self.mean, self.std = tuple(mean), tuple(std)
        self.resize_to, self.crop = resize_to, crop
        self.compute_dtype = compute_dtype
        self.last_terms = {}
        self.last_style_terms = {}
        self._tables = {}

    # ------------------------------------------------------------------ input
    def _check_size(self, h, w):
        for k in range(self.depth - 1):                           # a pool behind the deepest tap does not run
            if k in _POOL_AFTER:
                if h % 2 or w % 2 or h < 2 or w < 2:
                    raise ValueError(f"VggFeatureLoss: the {h} x {w} map in front of the max-pool after convolution {k + 1} is "
                                     "odd; pad or crop the images (or give resize_to and crop)")
                h, w = h // 2, w // 2

    def tables(self, h, w, device):
        key = (h, w, str(device))
        if key not in self._tables:
            if self.resize_to is None:
                self._check_size(h, w)
                self._tables[key] = _IdentityTables(h, w, device, self.mean, self.std)
            else:
                self._tables[key] = _G.ResampleTables(h, w, device, self.resize_to, self.crop, self.mean, self.std)
        return self._tables[key]

    def _input(self, image):
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"VggFeatureLoss: images are [N, 3, H, W], got {tuple(image.shape)}")
        return F.ResizeNorm.apply(image, self.tables(image.shape[2], image.shape[3], image.device), self.compute_dtype)

    # ------------------------------------------------------------------ trunk
    def _convs(self):
        return [m for m in self.net[0].children() if isinstance(m, nn.Conv2d)][:self.depth]

    def _run(self, x, targets, grams=None):
        """The trunk up to the deepest tap.  targets None: the target's half (no gradient), returns the tuple of taps.
        Otherwise: the tuple of taps of the other image; returns the per-tap means in tap order.  grams: the target's Gram
        matrices, for a style-weighted module; the return is then (content means or Nones, style means)."""
        tapped = {(o, post): i for i, (o, post, _, _) in enumerate(self.taps)}
        out = [None] * len(self.taps)
        sout = [None] * len(self.taps)
        content = self.perceptual_weight > 0.0

        def tap(y, i, need_relu, c):
            if grams is None:
                return F.FeatureTap.apply(y, targets[i], self.mode, need_relu, c) + (None,)
            return F.FeatureStyleTap.apply(y, targets[i] if content else None, grams[i], self.mode, need_relu, c, content)
        link = None                   # the Handover of the activation that produced x (see Vgg19Loss.features)
        for k, m in enumerate(self._convs()):
            pre, post = tapped.get((k, False)), tapped.get((k, True))
            last = k == self.depth - 1
            if pre is not None:
                # the convolution alone; the tap's pass writes the ReLU for the next layer and its backward applies that
                # ReLU's mask to the gradient coming back, in the launch that adds the tap's own term
                y = F.ConvAct.apply(x, m.weight, m.bias, None, dict(stride=1, pad=1, act=F.ACT_NONE, in_link=link))
                need_relu = post is not None or not last
                if targets is None:
                    out[pre] = y
                    x = F.relu16(y) if need_relu else y
                else:
                    x, out[pre], sout[pre] = tap(y, pre, need_relu, m.out_channels)
                link = None
            else:
                # a relu tap gives the activation two consumers, so the Handover chain ends at that layer: it runs its own
                # activation backward on the sum the tap hands back
                out_link = F.Handover() if post is None else None
                x = F.ConvAct.apply(x, m.weight, m.bias, None,
                                    dict(stride=1, pad=1, act=F.ACT_RELU, in_link=link, out_link=out_link))
                link = out_link
            if post is not None:
                if targets is None:
                    out[post] = x
                else:
                    x, out[post], sout[post] = tap(x, post, False, m.out_channels)
                link = None
            if k in _POOL_AFTER and not last:
                x = F.MaxPool2.apply(x, link)
                link = None
        return tuple(out) if grams is None else (tuple(out), tuple(sout))

    def target_features(self, image):
        """The 16-bit NHWC taps of the target, in trunk order (``layer_names``), computed without a gradient."""
        with torch.no_grad():
            return self._run(self._input(image), None)

    def target_grams(self, features2):
        """The fp32 [N, C, C] Gram matrices of the target's taps (``target_features``), in trunk order, without a gradient."""
        features2 = tuple(features2)
        if len(features2) != len(self.taps):
            raise ValueError(f"VggFeatureLoss: features2 holds {len(features2)} maps, the module has {len(self.taps)} taps")
        convs = self._convs()
        with torch.no_grad():
            return tuple(F.gram16(t, convs[o].out_channels) for t, (o, _, _, _) in zip(features2, self.taps))

    def _targets(self, image2, features2, grams2):
        if image2 is not None and image2.requires_grad:
            raise ValueError("VggFeatureLoss: image2 is the target and gets no gradient; detach it (only image1 is differentiated)")
        if features2 is None:
            features2 = self.target_features(image2)
        features2 = tuple(features2)
        if len(features2) != len(self.taps):
            raise ValueError(f"VggFeatureLoss: features2 holds {len(features2)} maps, the module has {len(self.taps)} taps")
        if self.style_weight > 0.0:
            grams2 = self.target_grams(features2) if grams2 is None else tuple(grams2)
            if len(grams2) != len(self.taps):
                raise ValueError(f"VggFeatureLoss: grams2 holds {len(grams2)} matrices, the module has {len(self.taps)} taps")
        else:
            grams2 = None
        return features2, grams2

    def terms(self, image1, image2, features2=None, grams2=None):
        """(percep, style): the two weighted halves of the loss, None for a zero weight."""
        features2, grams2 = self._targets(image2, features2, grams2)
        if grams2 is None:
            values, svalues = self._run(self._input(image1), features2), None
        else:
            values, svalues = self._run(self._input(image1), features2, grams2)
        percep = style = None
        self.last_terms, self.last_style_terms = {}, {}
        if self.perceptual_weight > 0.0:
            self.last_terms = {name: v.detach() for name, v in zip(self.layer_names, values)}
            percep = F.weighted_sum(values, [self.perceptual_weight * w for _, _, _, w in self.taps])
        if svalues is not None:
            self.last_style_terms = {name: v.detach() for name, v in zip(self.layer_names, svalues)}
            style = F.weighted_sum(svalues, [self.style_weight * w for _, _, _, w in self.taps])
        return percep, style

    def forward(self, image1, image2, features2=None, grams2=None):
        percep, style = self.terms(image1, image2, features2, grams2)
        if percep is None or style is None:
            return style if percep is None else percep
        return F.add_losses(percep, style)
