"""SRVGGNetCompact, Real-ESRGAN's compact generator (Wang et al. 2021), computed by the HIP kernels.

Written from BasicSR's published definition of the network: same class name, constructor arguments and child-module names,
therefore the same ``state_dict`` keys and shapes as the checkpoints people have on disk (``realesr-general-x4v3.pth``,
``realesr-general-wdn-x4v3.pth``: num_conv 32; ``realesr-animevideov3.pth``, ``RealESRGANv2-animevideo-*``: num_conv 16;
``evaluate.load_model`` unwraps their ``params_ema`` / ``params``, ``evaluate.inspect_srvgg`` reads the constructor arguments
off a file).  Parity with BasicSR and with trained weights is UNPINNED: neither was available to compare against; the tests
pin this file to a float64 restatement of the definition (tests/compact_ref.py).

    body.0                 Conv2d(num_in_ch, num_feat, 3, 1, 1)         body.1               activation
    body.{2k+2}            Conv2d(num_feat, num_feat, 3, 1, 1)          body.{2k+3}          activation      k < num_conv
    body.{2 num_conv + 2}  Conv2d(num_feat, num_out_ch * upscale^2, 3, 1, 1)
    forward                pixel_shuffle(body(x), upscale) + nearest_upsample(x, upscale)        no output activation

act_type: 'prelu' = nn.PReLU(num_parameters=num_feat) (initial value 0.25; key ``body.{odd}.weight`` of shape [num_feat]),
'relu', 'leakyrelu' (slope 0.1).  A departure from BasicSR: the add needs num_in_ch == num_out_ch (BasicSR would broadcast
or fail at run time); here anything else is a ValueError at construction.  upscale: an integer in 1..4.

The child modules are parameter holders only, as in rrdbnet.py.  Input and output are fp32 NCHW.  Two forms:
  * fused (grad mode off, or nothing that requires a gradient; num_feat 64: functional.compact_supported): ToNHWC, the head,
    num_conv launches of dsr_conv_prelu_c_fwd (conv + per-channel PReLU in the epilogue, the slope vector read from the
    parameter's own storage by every launch, so a HIP-graph replay after an optimiser step uses the new slopes) and one launch
    of dsr_conv_shuffle_add_fwd (conv + PixelShuffle + the fp32 input image, stored as fp32 NCHW).  The head (num_in_ch -> 64
    from 8 stored channels) is NOT that kernel: it runs as dsr_conv_fwd with no activation followed by one pointwise
    dsr_pw_prelu_c_fwd pass -- one extra pass out of num_conv + 2 layers;
  * composed (autograd; other widths; DSR_COMPACT_FUSED=0, read per call): per layer ConvAct with no activation, then
    functional.PReLUChannel, which saves the pre-activation; the tail is ConvOutNCHW followed by functional.ShuffleAdd.  It
    trains through the existing input- and weight-gradient kernels.  Correct, not tuned.
The two forms differ by one rounding per body layer: the composed form stores r16(slope * r16(v)), the fused one
r16(slope * v) (the head has the composed form's rounding in both).
'relu' and 'leakyrelu' run the same kernels with a constant slope vector (0 or 0.1) held as a non-persistent buffer: the
state_dict has no extra key.
Every PReLU backward takes its branch from the stored pre-activation, so slopes of any sign train exactly and this module
needs no ``functional.check_prelu_slopes`` (that check is for one-parameter PReLUs feeding output-masked launches).
No form reads anything on the host, so all replay from a HIP graph.
"""
import torch
import torch.nn as nn

from ... import functional as F

LEAKY_SLOPE = 0.1


class SRVGGNetCompact(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type='prelu'):
        super(SRVGGNetCompact, self).__init__()
        if act_type not in ('prelu', 'relu', 'leakyrelu'):
            raise ValueError(f"SRVGGNetCompact: act_type must be 'prelu', 'relu' or 'leakyrelu', got {act_type!r}")
        if isinstance(upscale, bool) or not isinstance(upscale, int) or not 1 <= upscale <= 4:
            raise ValueError(f"SRVGGNetCompact: upscale must be an integer in 1..4, got {upscale!r}")
        if num_in_ch != num_out_ch:
            raise ValueError(f"SRVGGNetCompact: the input image is added to the output, so num_in_ch ({num_in_ch}) must equal "
                             f"num_out_ch ({num_out_ch})")
        if num_in_ch < 1 or num_feat < 1 or num_conv < 0:
            raise ValueError("SRVGGNetCompact: num_in_ch and num_feat must be positive, num_conv non-negative")
        self.num_in_ch, self.num_out_ch, self.num_feat, self.num_conv = num_in_ch, num_out_ch, num_feat, num_conv
        self.upscale = upscale
        self.scale = upscale                    # infer._factor reads it
        self.act_type = act_type
        self.compute_dtype = torch.bfloat16     # float16 is accepted too

        def act():
            if act_type == 'prelu':
                return nn.PReLU(num_parameters=num_feat)
            return nn.ReLU(inplace=True) if act_type == 'relu' else nn.LeakyReLU(negative_slope=LEAKY_SLOPE, inplace=True)

        self.body = nn.ModuleList()
        self.body.append(nn.Conv2d(num_in_ch, num_feat, 3, 1, 1))
        self.body.append(act())
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(num_feat, num_feat, 3, 1, 1))
            self.body.append(act())
        self.body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        if act_type != 'prelu':
            const = 0.0 if act_type == 'relu' else LEAKY_SLOPE
            self.register_buffer("_const_slope", torch.full((num_feat,), const, dtype=torch.float32), persistent=False)

    def receptive_halo(self):
        """Input pixels of context a tile needs for its interior to equal the whole-image result: one per convolution."""
        return self.num_conv + 2

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _slope(self, k):
        """The slope vector of activation k (module body.{2k+1})."""
        return self.body[2 * k + 1].weight if self.act_type == 'prelu' else self._const_slope

    def forward(self, x):
        x = x.float()
        if x.dim() != 4 or x.shape[1] != self.num_in_ch:
            raise ValueError(f"SRVGGNetCompact: an [N,{self.num_in_ch},H,W] image is expected, got {tuple(x.shape)}")
        x = x.contiguous()
        cfg = dict(stride=1, pad=1, act=F.ACT_NONE)
        xi = F.ToNHWC.apply(x, self.compute_dtype)
        last = self.body[2 * self.num_conv + 2]
        if not self._wants_grad(x) and F.compact_supported(xi.shape, xi.dtype, self.num_feat, self.num_out_ch, self.upscale):
            feat = F.ConvAct.apply(xi, self.body[0].weight, self.body[0].bias, None, cfg)
            feat = F.prelu_channel(feat, self._slope(0).detach())
            for k in range(1, self.num_conv + 1):
                conv = self.body[2 * k]
                feat = F.compact_conv(feat, conv.weight, conv.bias.detach(), self._slope(k).detach())
            return F.compact_tail(feat, last.weight, last.bias.detach(), x, self.upscale)
        feat = xi
        for k in range(self.num_conv + 1):
            conv = self.body[2 * k]
            feat = F.PReLUChannel.apply(F.ConvAct.apply(feat, conv.weight, conv.bias, None, cfg), self._slope(k))
        t = F.ConvOutNCHW.apply(feat, last.weight, last.bias, cfg)
        return F.ShuffleAdd.apply(t, x, self.upscale)
