"""UNetDiscriminatorSN, the Real-ESRGAN discriminator (Wang et al. 2021), computed by the HIP kernels.

Written from BasicSR's published definition of the network: a U-Net of spectrally normalised convolutions that returns one
logit per pixel.  Same class name, constructor arguments and child-module names, and the state_dict layout of
``torch.nn.utils.spectral_norm`` (``convK.weight_orig`` a Parameter, ``convK.weight_u`` / ``convK.weight_v`` buffers, no
``convK.weight``), therefore the keys and shapes of ``RealESRGAN_x4plus_netD.pth``.  Parity with BasicSR and with trained
weights is UNPINNED: neither was available to compare against; the tests pin this file to a float64 restatement of the
definition (tests/unetd_ref.py) and the spectral norm to ``torch.nn.utils.spectral_norm`` itself (tests/spectral_ref.py).

    x0 = lrelu(conv0(x))                                      3x3, bias
    x1 = lrelu(conv1(x0)); x2 = lrelu(conv2(x1)); x3 = lrelu(conv3(x2))        SN 4x4 stride 2 pad 1, no bias
    x4 = lrelu(conv4(up(x3))) + x2;  x5 = lrelu(conv5(up(x4))) + x1;  x6 = lrelu(conv6(up(x5))) + x0      SN 3x3, no bias
    out = conv9(lrelu(conv8(lrelu(conv7(x6)))))               SN 3x3, SN 3x3, 3x3 with bias: [N, 1, H, W] logits

LeakyReLU slope 0.2, `up` = bilinear x2 with align_corners=False, the additions only with skip_connection.

In train mode every forward advances the power iteration of all eight normalised layers (u and v are rewritten on the
device, inside one launch group that goes out before the first convolution); eval mode reads the stored vectors.  Nothing is
read on the host, so the module replays from a HIP graph and every replay advances the iteration, as an eager call does.
"""
import torch
import torch.nn as nn
import torch.nn.functional as TF

from ... import functional as F

SLOPE = 0.2
SN_LAYERS = tuple(f"conv{i}" for i in range(1, 9))


class _SNConv(nn.Module):
    """Parameter holder of ``spectral_norm(nn.Conv2d(cin, cout, k, stride, 1, bias=False))``: weight_orig, weight_u, weight_v."""

    def __init__(self, cin, cout, k, stride):
        super().__init__()
        conv = nn.Conv2d(cin, cout, k, stride, 1, bias=False)              # (its default initialisation)
        self.weight_orig = nn.Parameter(conv.weight.detach().clone())
        # torch's hook: u and v start as normalised standard-normal vectors
        self.register_buffer("weight_u", TF.normalize(torch.randn(cout), dim=0, eps=F.SN_EPS))
        self.register_buffer("weight_v", TF.normalize(torch.randn(cin * k * k), dim=0, eps=F.SN_EPS))
        self.stride = stride


class UNetDiscriminatorSN(nn.Module):
    def __init__(self, num_in_ch=3, num_feat=64, skip_connection=True):
        super(UNetDiscriminatorSN, self).__init__()
        nf = num_feat
        self.skip_connection = skip_connection
        self.conv0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.conv1 = _SNConv(nf, nf * 2, 4, 2)
        self.conv2 = _SNConv(nf * 2, nf * 4, 4, 2)
        self.conv3 = _SNConv(nf * 4, nf * 8, 4, 2)
        self.conv4 = _SNConv(nf * 8, nf * 4, 3, 1)
        self.conv5 = _SNConv(nf * 4, nf * 2, 3, 1)
        self.conv6 = _SNConv(nf * 2, nf, 3, 1)
        self.conv7 = _SNConv(nf, nf, 3, 1)
        self.conv8 = _SNConv(nf, nf, 3, 1)
        self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)
        self.compute_dtype = torch.bfloat16     # float16 is accepted too

    def normalised_weights(self):
        """The eight W_sn of this forward, in layer order: one launch group for all the iterations."""
        layers = [getattr(self, name) for name in SN_LAYERS]
        return F.spectral_norm_weights([m.weight_orig for m in layers], [m.weight_u for m in layers],
                                       [m.weight_v for m in layers], self.training)

    def forward(self, x):
        if x.dim() != 4 or x.shape[-2] % 8 or x.shape[-1] % 8:
            raise ValueError(f"UNetDiscriminatorSN: the input must be [N, C, H, W] with H and W multiples of 8 (the skip "
                             f"connections meet three stride-2 layers), got {tuple(x.shape)}")
        F._need_gpu(x)
        w = dict(zip(SN_LAYERS, self.normalised_weights()))

        def conv(v, name):
            return F.ConvAct.apply(v, w[name], None, None, dict(stride=getattr(self, name).stride, pad=1, act=F.ACT_LEAKY,
                                                                slope=SLOPE))

        def up(v):
            return F.Bilinear2x.apply(v)

        def add(a, b):
            return F.ScaleAdd.apply(a, 1.0, b) if self.skip_connection else a

        xi = F.ToNHWC.apply(x, self.compute_dtype)
        x0 = F.ConvAct.apply(xi, self.conv0.weight, self.conv0.bias, None, dict(stride=1, pad=1, act=F.ACT_LEAKY, slope=SLOPE))
        x1 = conv(x0, "conv1")
        x2 = conv(x1, "conv2")
        x3 = conv(x2, "conv3")
        x4 = add(conv(up(x3), "conv4"), x2)
        x5 = add(conv(up(x4), "conv5"), x1)
        x6 = add(conv(up(x5), "conv6"), x0)
        out = conv(conv(x6, "conv7"), "conv8")
        return F.ConvOutNCHW.apply(out, self.conv9.weight, self.conv9.bias, dict(stride=1, pad=1, act=F.ACT_NONE))
