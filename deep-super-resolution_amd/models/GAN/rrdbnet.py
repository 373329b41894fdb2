"""RRDBNet, the ESRGAN / Real-ESRGAN generator (Wang et al. 2018, 2021), computed by the HIP kernels.

Written from BasicSR's published definition of the network (the reference this package mirrors only has the SRGAN
generator, generator.py): same class names, constructor arguments and child-module names, therefore the same
``state_dict`` keys and shapes as the checkpoints people have on disk (``RealESRGAN_x4plus.pth``, ``RealESRGAN_x2plus.pth``,
``ESRGAN_SRx4_DF2KOST_official.pth`` in BasicSR's format; ``evaluate.load_model`` unwraps their ``params_ema`` / ``params``).
Parity with BasicSR is UNPINNED: neither the package nor trained weights were available to compare against; the tests pin
this file to a float64 restatement of the definition (tests/rrdb_ref.py).

    ResidualDenseBlock   x1 = lrelu(conv1(x)); x2 = lrelu(conv2(cat(x, x1))); ... x5 = conv5(cat(x, x1..x4)); x5 * 0.2 + x
    RRDB                 rdb3(rdb2(rdb1(x))) * 0.2 + x
    RRDBNet              feat = conv_first(pixel_unshuffle(x, 2 | 4 for scale 2 | 1));  feat += conv_body(body(feat));
                         feat = lrelu(conv_up1(nearest2x(feat))); feat = lrelu(conv_up2(nearest2x(feat)));
                         conv_last(lrelu(conv_hr(feat)))               LeakyReLU slope 0.2 throughout, no output activation

The child nn.Conv2d objects are parameter holders only, as in generator.py.  Two forms of the body:
  * fused (grad mode off, or nothing that requires a gradient): every dense block is five launches of
    functional.rdb_forward on three rotating "growth buffers" [N,H,W,num_feat + 4 num_grow_ch] -- no concatenation copy, the
    residual scalings ride in conv5's epilogue (csrc/conv_rdb.hip);
  * composed (autograd): ConvAct / ConcatChannels / ScaleAdd, which trains through the existing input- and weight-gradient
    kernels.  Channel counts the fused kernel does not take (anything but num_feat 64, num_grow_ch 32), and
    DSR_RRDB_FUSED=0, take this form without a gradient too;
  * fused training (autograd, opt-in: ``net.set_fused_training()``): the whole body is one functional.RRDBBody node -- the
    fused forward with one growth buffer per dense block kept as the saved activations, and a backward that runs on
    gradient buffers of the same shape (csrc/conv_rdb.hip's input-gradient form, csrc/conv_rdb_bwd.hip).  Same forward
    bits as the fused form; taken where functional.rdb_train_supported says so, else the composed form.
No form reads anything on the host, so all replay from a HIP graph.
"""
import torch
import torch.nn as nn
import torch.nn.functional as TF

from ... import functional as F

SLOPE = 0.2      # every LeakyReLU of the network
BETA = 0.2       # residual scaling of a dense block and of an RRDB


def _conv(x, conv, act):
    return F.ConvAct.apply(x, conv.weight, conv.bias, None, dict(stride=1, pad=1, act=act, slope=SLOPE))


class ResidualDenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super(ResidualDenseBlock, self).__init__()
        self.conv1 = nn.Conv2d(num_feat, num_grow_ch, 3, 1, 1)
        self.conv2 = nn.Conv2d(num_feat + num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv3 = nn.Conv2d(num_feat + 2 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv4 = nn.Conv2d(num_feat + 3 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)
        self.num_feat, self.num_grow_ch = num_feat, num_grow_ch
        for conv in self._convs():                      # Kaiming-normal x 0.1, zero bias
            nn.init.kaiming_normal_(conv.weight)
            with torch.no_grad():
                conv.weight.mul_(0.1)
                conv.bias.zero_()

    def _convs(self):
        return (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5)

    def _composed(self, x):
        nf, gc = self.num_feat, self.num_grow_ch
        xs = [x]
        for k, conv in enumerate(self._convs()):
            inp = x if k == 0 else F.ConcatChannels.apply((nf,) + (gc,) * k, *xs)
            y = _conv(inp, conv, F.ACT_LEAKY if k < 4 else F.ACT_NONE)
            xs.append(y)
        return F.ScaleAdd.apply(xs[5], BETA, x)

    def _fused(self, buf_in, buf_out, res2=None):
        convs = self._convs()
        F.rdb_forward(buf_in, [c.weight for c in convs], [c.bias for c in convs], buf_out, res2=res2, slope=SLOPE, beta=BETA)


class RRDB(nn.Module):
    def __init__(self, num_feat, num_grow_ch=32):
        super(RRDB, self).__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)

    def _composed(self, x):
        out = self.rdb3._composed(self.rdb2._composed(self.rdb1._composed(x)))
        return F.ScaleAdd.apply(out, BETA, x)


class RRDBNet(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
        super(RRDBNet, self).__init__()
        if scale not in (1, 2, 4):
            raise ValueError(f"RRDBNet: scale must be 1, 2 or 4, got {scale}")
        self.scale = scale
        self.unshuffle = {4: 1, 2: 2, 1: 4}[scale]       # pixel_unshuffle factor in front of conv_first
        self.conv_first = nn.Conv2d(num_in_ch * self.unshuffle ** 2, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self.num_feat, self.num_grow_ch = num_feat, num_grow_ch
        self.compute_dtype = torch.bfloat16     # float16 is accepted too
        self.fused_training = False             # a plain attribute (not in the state_dict): see set_fused_training

    def set_fused_training(self, on=True):
        """Train the body on its growth buffers (functional.RRDBBody) where the kernels take the shape; returns self."""
        self.fused_training = bool(on)
        return self

    def receptive_halo(self):
        """Input pixels of context a tile needs for its interior to equal the whole-image result: conv_first and conv_body
        (2), 15 convs per RRDB, and conv_up1 / conv_up2 / conv_hr / conv_last at 2x and 4x (1/2 + 1/4 + 1/4 + 1/4, rounded
        up to 2) -- in pixels of the feature grid, times the pixel_unshuffle factor."""
        return (2 + 15 * len(self.body) + 2) * self.unshuffle

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _body_fused(self, feat):
        n, h, w, _ = feat.shape
        nf = self.num_feat
        bufs = [torch.empty((n, h, w, nf + 4 * self.num_grow_ch), dtype=feat.dtype, device=feat.device) for _ in range(3)]
        F._box_copy(feat, bufs[0], n, h, w, nf, 0, 0, 0, 0, 0, 0)
        out = None
        for i, block in enumerate(self.body):
            # three buffers rotate: the RRDB's input a (kept for its outer residual), b, c; its result lands in b
            a, b, c = bufs[i % 3], bufs[(i + 1) % 3], bufs[(i + 2) % 3]
            block.rdb1._fused(a, b)
            block.rdb2._fused(b, c)
            if i + 1 == len(self.body):
                out = torch.empty((n, h, w, nf), dtype=feat.dtype, device=feat.device)
                block.rdb3._fused(c, out, res2=a)
            else:
                block.rdb3._fused(c, b, res2=a)
        return out

    def _body_train(self, feat):
        params = []
        for block in self.body:
            for rdb in (block.rdb1, block.rdb2, block.rdb3):
                for conv in rdb._convs():
                    params += [conv.weight, conv.bias]
        return F.RRDBBody.apply(feat, dict(slope=SLOPE, beta=BETA), *params)

    def forward(self, x):
        f = self.unshuffle
        if f > 1:
            if x.shape[-2] % f or x.shape[-1] % f:
                raise ValueError(f"RRDBNet(scale={self.scale}): H and W must be multiples of {f}, got {tuple(x.shape[-2:])}")
            x = TF.pixel_unshuffle(x.float(), f)
        xi = F.ToNHWC.apply(x, self.compute_dtype)
        feat = _conv(xi, self.conv_first, F.ACT_NONE)
        if len(self.body) == 0:
            body = feat
        elif not self._wants_grad(x) and F.rdb_supported(feat.shape, feat.dtype, self.num_feat, self.num_grow_ch):
            body = self._body_fused(feat)
        elif self.fused_training and F.rdb_train_supported(feat.shape, feat.dtype, self.num_feat, self.num_grow_ch):
            body = self._body_train(feat)
        else:
            body = feat
            for block in self.body:
                body = block._composed(body)
        feat = F.ScaleAdd.apply(_conv(body, self.conv_body, F.ACT_NONE), 1.0, feat)
        feat = _conv(F.Nearest2x.apply(feat), self.conv_up1, F.ACT_LEAKY)
        feat = _conv(F.Nearest2x.apply(feat), self.conv_up2, F.ACT_LEAKY)
        feat = _conv(feat, self.conv_hr, F.ACT_LEAKY)
        return F.ConvOutNCHW.apply(feat, self.conv_last.weight, self.conv_last.bias, dict(stride=1, pad=1, act=F.ACT_NONE))
