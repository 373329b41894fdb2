"""The timed step recipes on the HIP path.

gen_l1_step : BASELINE config 2 (generator-only x4, L1, Adam) -- defined by SURVEY.md 8(d).
gen_lpips_step : the same step with the perceptual fine-tuning loss l1_weight * L1 + lpips_weight * LPIPS(fake, hr).
gen_msssim_step : the same step with the structural loss alpha * (1 - MS-SSIM(fake, hr)) + (1 - alpha) * L1.
gen_perceptual_step : the same step with the content loss l1_weight * L1 + VggFeatureLoss(fake, hr) (ESRGAN / Real-ESRGAN).
gan_step    : train_GAN.py:38-71 (do_epoch): D step, then G step with the detached adversarial term.
realesrgan_step : the GAN stage of Real-ESRGAN (L1 + VGG features + a logits GAN loss whose gradient flows through D into G).
esrgan_step : the GAN stage of ESRGAN (the same terms under the relativistic average discriminator, five D forwards).
dip_step   : DIP.py:47-95 closure + utils/DIP.py:33-40 Adam iteration.
"""
import contextlib
import os

import torch

from . import functional as F


def _backward_and_step(loss, opt, scaler, ema=None):
    """loss.backward(); opt.step() -- under an optim.DynamicLossScaler: scaled loss, checked and predicated step, update.
    `ema` (an optim.WeightEMA): averaged right after the optimizer's step, while the scaler's overflow flag of this step is
    still up -- a skipped step leaves the average alone too."""
    with F.batched_wgrad():              # e.g. the 35 3x3 weight gradients of the generator: one grouped launch at the end
        (loss if scaler is None else scaler.scale(loss)).backward()
    if scaler is None:
        opt.step()
        if ema is not None:
            ema.update()
    else:
        scaler.step(opt)
        if ema is not None:
            ema.update(scaler)
        scaler.update()


@contextlib.contextmanager
def _requires_grad(params, flag):
    """Every parameter's requires_grad set to `flag` inside the block; the flags found on entry are put back on exit."""
    was = [p.requires_grad for p in params]
    for p in params:
        p.requires_grad_(flag)
    try:
        yield
    finally:
        for p, r in zip(params, was):
            p.requires_grad_(r)


def gen_l1_step(gen, opt, lr_patches, hr_patches, *, scaler=None, ema=None):
    """`scaler`: an optim.DynamicLossScaler for a generator with fp16 storage (the default bf16 needs none).  `ema`: an
    optim.WeightEMA over the generator, updated after the optimizer's step (here and in the recipes below)."""
    fake = gen(lr_patches)
    loss = F.l1_loss(fake, hr_patches)
    opt.zero_grad()
    _backward_and_step(loss, opt, scaler, ema)
    return loss.detach(), fake.detach()


def gen_lpips_step(gen, opt, lpips, lr_patches, hr_patches, l1_weight=1.0, lpips_weight=0.1, *, scaler=None, ema=None):
    """Perceptual fine-tuning of a PSNR-trained generator: loss = l1_weight * L1 + lpips_weight * LPIPS(fake, hr).

    `lpips`: an lpips.LPIPS with normalize=False (the generator ends in tanh and scale_images targets live in [-1, 1]); only
    `fake` requires a gradient, so the LPIPS backward runs on that half of the trunk's batch.  Returns the two unweighted terms
    and `fake` as device tensors (no host sync here).  Inside GraphedStep the module needs validate_range=False: the range
    check is the one host read of the call.  `scaler`: an optim.DynamicLossScaler around the summed loss (the LPIPS trunk
    keeps its own internal grad_scale)."""
    fake = gen(lr_patches)
    l1 = F.l1_loss(fake, hr_patches)
    lp = lpips(fake, hr_patches)
    loss = F.add_losses(F.scale_loss(l1, float(l1_weight)), F.scale_loss(lp, float(lpips_weight)))
    opt.zero_grad()
    _backward_and_step(loss, opt, scaler, ema)
    return l1.detach(), lp.detach(), fake.detach()


def gen_msssim_step(gen, opt, msssim, lr_patches, hr_patches, alpha=0.84, *, scaler=None, ema=None):
    """The structural loss of Zhao, Gallo, Frosio, Kautz 2017: loss = alpha * (1 - MS-SSIM(fake, hr)) + (1 - alpha) * L1.

    `msssim`: a metrics.MultiScaleStructuralSimilarityIndexMeasure with reduction 'elementwise_mean' or 'sum' whose data_range
    spans the images (2.0 for a tanh generator and scale_images targets in [-1, 1]); the patches must be at least its min_size
    on a side (176 for the default five scales).  Only `fake` requires a gradient, so each scale's backward writes one image's
    gradient.  Returns the two unweighted terms (1 - MS-SSIM, L1) and `fake` as device tensors (no host sync here); usable
    inside GraphedStep.  `scaler`: an optim.DynamicLossScaler around the summed loss."""
    fake = gen(lr_patches)
    l1 = F.l1_loss(fake, hr_patches)
    dis = F.one_minus(msssim(fake, hr_patches))
    loss = F.add_losses(F.scale_loss(dis, float(alpha)), F.scale_loss(l1, 1.0 - float(alpha)))
    opt.zero_grad()
    _backward_and_step(loss, opt, scaler, ema)
    return dis.detach(), l1.detach(), fake.detach()


def gen_perceptual_step(gen, opt, vggfeat, lr_patches, hr_patches, l1_weight=1.0, *, scaler=None, ema=None):
    """The pixel + content loss of the ESRGAN / Real-ESRGAN recipes (without the adversarial term):
    loss = l1_weight * L1 + vggfeat(fake, hr).

    `vggfeat`: a perceptual.VggFeatureLoss; its layer weights and perceptual_weight are the content term's whole weighting.
    Build it with range_norm=True for a tanh generator and scale_images targets in [-1, 1].  Only `fake` requires a gradient.
    A module built with style_weight > 0 is taken as it is: the content term returned here (and by realesrgan_step and
    gan_step) then includes its style term.
    Returns the unweighted L1 term, the (weighted) content term and `fake` as device tensors (no host sync here); usable
    inside GraphedStep.  `scaler`: an optim.DynamicLossScaler around the summed loss (needed for compute_dtype=float16: the
    feature loss keeps no gradient scale of its own)."""
    fake = gen(lr_patches)
    l1 = F.l1_loss(fake, hr_patches)
    pc = vggfeat(fake, hr_patches)
    loss = F.add_losses(F.scale_loss(l1, float(l1_weight)), pc)
    opt.zero_grad()
    _backward_and_step(loss, opt, scaler, ema)
    return l1.detach(), pc.detach(), fake.detach()


_side_streams = {}


def _side_stream(device, which="d"):
    key = (device.type, device.index, which)
    if key not in _side_streams:
        # DSR_SIDE_PRIORITY (tuning switch): HIP stream priority of the D-half stream, 0 = default, -1 = high
        _side_streams[key] = torch.cuda.Stream(device=device, priority=int(os.environ.get("DSR_SIDE_PRIORITY", "0")))
    return _side_streams[key]


TRACE = None    # development aid: a list -> gan_step appends (label, event recorded on the stream that reached that point)


def _mark(label, stream):
    if TRACE is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        TRACE.append((label, ev))


def gan_step(gen, disc, perceptual, opt_g, opt_d, lr_patches, hr_patches, sync_g=None, sync_d=None, overlap=True,
             batch_wgrad=None, ema=None):
    """train_GAN.py:38-71.  Returns (loss_D, loss_G, fake) as device tensors (no host sync here).

    Once `fake` exists the reference's two halves are independent: the D step (:44-53) reads only `fake.detach()`,
    and the G step's gradient comes only from the VGG content term -- the adversarial term is computed from a
    DETACHED generator output (:58), so it contributes a number to loss_G (:59) and nothing to loss_G.backward()
    (:63).  With `overlap` the D step (+ the no_grad D pass that feeds that number) runs on a second HIP stream
    while VGG forward/backward, the generator backward and its Adam run on the main one: the HBM-bound BatchNorm /
    Adam passes of one half execute under the MFMA-bound convolutions of the other.  The arithmetic is unchanged.
    `ema`: an optim.WeightEMA over the generator, updated after opt_g.step() on the main stream."""
    # train_GAN.py:46 and :56 evaluate gen(lr_patches) twice with the same weights and batch statistics -- the
    # two outputs are bit-identical and only the BatchNorm running statistics notice the second call.  One forward
    # (with the autograd graph the G step needs) + a double running-stat update is exactly equivalent.
    if batch_wgrad is None:
        batch_wgrad = os.environ.get("DSR_WGRAD_BATCH", "1") != "0"    # tuning switch: 0 = one weight-gradient launch per layer
    main = torch.cuda.current_stream(hr_patches.device)
    side = _side_stream(hr_patches.device) if overlap else main
    hr_feat = real_feat = None
    _mark("start", main)
    if overlap:
        # the VGG features of the HR target depend on nothing but the batch: they run beside the generator forward
        side.wait_stream(main)
        with torch.cuda.stream(side):
            hr_feat = perceptual.vgg_loss.target_features(hr_patches)
            hr_feat_ready = torch.cuda.Event()
            hr_feat_ready.record(side)
            # ... and so does D's conv trunk on the real batch (:44): same weights, same BatchNorm bookkeeping order
            # (real before fake) as in the reference, just started while the generator is still running
            real_feat = disc.features(hr_patches)
            _mark("side: HR VGG features + D(real) trunk done", side)
    gen.bn_updates = 2
    fake = gen(lr_patches)                                       # :46 and :56
    gen.bn_updates = 1
    _mark("main: G forward done", main)
    fake_det = fake.detach()
    if overlap:
        side.wait_stream(main)                                   # `fake` is complete before D reads it

    def d_half():
        real_d, fake_d = disc.forward_pair(hr_patches, fake_det, fa=real_feat)   # :44, :47 (BN statistics per batch, as there)
        loss_d = F.add_losses(F.bce_const(real_d, 1.0), F.bce_const(fake_d, 0.0))  # :48, utils/GAN.py:101-105
        opt_d.zero_grad()                                        # :51 (gan_D.zero_grad())
        with F.batched_wgrad(batch_wgrad):                       # (D's stride-1 layers, real + generated batch summed)
            loss_d.backward()                                    # :52
        _mark("D: backward done", torch.cuda.current_stream())
        if sync_d is not None:
            sync_d()
        opt_d.step()                                             # :53
        _mark("D: Adam done", torch.cuda.current_stream())
        with torch.no_grad():
            # :58 detaches the generator output, so this D pass never sends a gradient anywhere that survives
            # (D's .grad from it is wiped by the next zero_grad, :51); it still updates D's BN running statistics.
            adv = perceptual.adversarial(disc(fake_det))         # the adversarial number of :59
        return loss_d.detach(), adv

    if overlap:
        with torch.cuda.stream(side):
            loss_d, adv = d_half()
            _mark("D half done (incl. adversarial pass)", side)
    else:
        loss_d, adv = d_half()
    # --- generator (main stream)
    if hr_feat is not None:
        main.wait_event(hr_feat_ready)   # only the target features are needed here, not the D half queued behind them
        for feat in (hr_feat if isinstance(hr_feat, (tuple, list)) else (hr_feat,)):     # (a multi-tap content loss: a tuple)
            feat.record_stream(main)
    content = perceptual.content(fake, hr_patches, hr_feat)      # the only term of :59 with a gradient path
    opt_g.zero_grad()                                            # :62
    _mark("main: VGG content loss forward done", main)
    # the generator's 35 3x3 layers: grouped launches.  With `overlap` every DSR_WGRAD_EARLY (default 16, 0 = off) collected
    # layers go out at once on a third stream: the generator half is the longer chain of the two, its backward is one long
    # dependency chain of input gradients, and the weight gradients hang off that chain -- launched at the exit they ran alone
    # at the end of the step (the D half has finished by then); launched as they become ready they run beside the chain
    early = int(os.environ.get("DSR_WGRAD_EARLY", "16")) if (overlap and batch_wgrad) else 0
    with F.batched_wgrad(batch_wgrad, early_stream=_side_stream(hr_patches.device, "wgrad") if early else None, early_every=early):
        content.backward()                                       # :63 (d adversarial / d generator == 0, see above)
    _mark("main: G backward done", main)
    if sync_g is not None:
        sync_g()
    opt_g.step()                                                 # :64
    if ema is not None:
        ema.update()
    _mark("main: G Adam done", main)
    if overlap:
        main.wait_stream(side)                                   # D half done before anything later on `main`
        loss_d.record_stream(main)
        adv.record_stream(main)
    loss_g = F.add_losses(content.detach(), adv)                  # :59 value (unweighted sum, utils/GAN.py:122)
    return loss_d, loss_g, fake_det


def realesrgan_step(gen, disc, vggfeat, opt_g, opt_d, lq, gt, *, l1_weight=1.0, gan_weight=0.1, gan_type="vanilla", ema=None,
                    gt_usm=None, l1_gt_usm=True, percep_gt_usm=True, gan_gt_usm=False, ldl_weight=0.0, gen_ema=None,
                    ldl_detach=False):
    """One GAN-stage step of the Real-ESRGAN recipe (BasicSR RealESRGANModel.optimize_parameters).  Unlike gan_step, the
    adversarial gradient flows through D into G.  With ``gt_usm=None`` `gt` is the target of all three terms.  With a tensor
    (``utils.degradation.usm_sharp(gt)``, the unsharp-masked ground truth) the L1 term, the content term and the
    discriminator's real pass each take `gt_usm` or `gt` by their flag `l1_gt_usm`, `percep_gt_usm`, `gan_gt_usm` (the
    published defaults); the launches are the same, only the tensors they read differ.

    Generator half, D frozen (no weight gradient and no spectral-norm backward runs for it):
        fake = gen(lq);  l_g = l1_weight * L1(fake, gt) + vggfeat(fake, gt) + gan_weight * gan_loss(disc(fake), real)
    Discriminator half: gan_loss(disc(gt), real, is_disc) and gan_loss(disc(fake.detach()), fake, is_disc), each with a
    backward of its own, then opt_d.step().

    `disc`: a models.GAN.UNetDiscriminatorSN (any module of fp32 NCHW in, logits out) and is left in the mode it came in;
    in train mode one step advances every u and v by three power iterations, as the published loop does.  Returns (l_pix,
    l_percep, l_g_gan, l_d_real, l_d_fake, fake): the unweighted L1, the (weighted) content term, the unweighted three GAN
    terms and the generator's output, as detached device tensors.  One stream, no host read: usable inside GraphedStep with a
    FusedAdam for each optimiser.

    ``ldl_weight > 0`` adds the LDL artifact term (BasicSR's ldl_opt, functional.ldl_loss) and needs ``gen_ema``, a second
    generator module that holds the averaged weights:
        fake_ema = gen_ema(lq)  (no gradient; the average as it stood BEFORE this step's update, the published order)
        l_g += ldl_weight * ldl_loss(fake, l1_gt, fake_ema, detach_weight=ldl_detach)
    The term takes the L1 term's target (gt_usm or gt by `l1_gt_usm`), as BasicSR's does.  After ``ema.update()`` the step writes
    the new average into `gen_ema` (``ema.copy_to(gen_ema)``) when both are given, and it returns a seven-tuple with the unweighted
    term appended: (l_pix, l_percep, l_g_gan, l_d_real, l_d_fake, fake, l_g_ldl).
    With ``ldl_weight == 0`` (the default) neither keyword is looked at: the launches, the bits and the six-tuple are as before."""
    ldl = float(ldl_weight)
    if ldl < 0.0 or ldl != ldl:
        raise ValueError(f"realesrgan_step: ldl_weight must be >= 0, got {ldl_weight!r}")
    if ldl > 0.0 and gen_ema is None:
        raise ValueError("realesrgan_step: ldl_weight > 0 needs gen_ema, a generator module holding the averaged weights")
    l1_gt = gt_usm if (gt_usm is not None and l1_gt_usm) else gt
    percep_gt = gt_usm if (gt_usm is not None and percep_gt_usm) else gt
    gan_gt = gt_usm if (gt_usm is not None and gan_gt_usm) else gt
    if ldl > 0.0:
        with torch.no_grad():
            fake_ema = gen_ema(lq)
    d_params = [p for p in disc.parameters()]
    # --- generator
    with _requires_grad(d_params, False):
        opt_g.zero_grad()
        fake = gen(lq)
        l_pix = F.l1_loss(fake, l1_gt)
        l_percep = vggfeat(fake, percep_gt)
        l_g_gan = F.gan_loss(disc(fake), True, gan_type, is_disc=False)
        l_g = F.add_losses(F.add_losses(F.scale_loss(l_pix, float(l1_weight)), l_percep), F.scale_loss(l_g_gan, float(gan_weight)))
        if ldl > 0.0:
            l_g_ldl = F.ldl_loss(fake, l1_gt, fake_ema, detach_weight=ldl_detach)
            l_g = F.add_losses(l_g, F.scale_loss(l_g_ldl, ldl))
        with F.batched_wgrad():
            l_g.backward()
        opt_g.step()
        if ema is not None:
            ema.update()
            if ldl > 0.0:
                ema.copy_to(gen_ema)
    # --- discriminator
    with _requires_grad(d_params, True):
        opt_d.zero_grad()
        l_d_real = F.gan_loss(disc(gan_gt), True, gan_type, is_disc=True)
        with F.batched_wgrad():
            l_d_real.backward()
        l_d_fake = F.gan_loss(disc(fake.detach()), False, gan_type, is_disc=True)
        with F.batched_wgrad():
            l_d_fake.backward()
        opt_d.step()
    out = (l_pix.detach(), l_percep.detach(), l_g_gan.detach(), l_d_real.detach(), l_d_fake.detach(), fake.detach())
    return out + (l_g_ldl.detach(),) if ldl > 0.0 else out


def esrgan_step(gen, disc, vggfeat, opt_g, opt_d, lq, gt, *, l1_weight=1e-2, gan_weight=5e-3, gan_type="vanilla", ema=None):
    """One GAN-stage step of the ESRGAN recipe (BasicSR ESRGANModel.optimize_parameters): realesrgan_step with the relativistic
    average discriminator.  Each logit is judged against the batch mean of the opposite class, rel(x, other, label) =
    F.relativistic_gan_loss, so D's gradient depends on both of its passes and G's adversarial gradient on the ground truth.

    Generator half, D frozen:
        real_pred = disc(gt) (no gradient);  fake_pred = disc(fake)
        l_g_gan = (rel(real_pred, fake_pred, fake) + rel(fake_pred, real_pred, real)) / 2
        l_g = l1_weight * L1(fake, gt) + vggfeat(fake, gt) + gan_weight * l_g_gan          (vggfeat=None: no content term)
    Discriminator half, in the published order:
        fake_pred = disc(fake.detach()) (no gradient);  real_pred = disc(gt)
        l_d_real = rel(real_pred, fake_pred, real, is_disc) / 2, backward
        fake_pred = disc(fake.detach());  l_d_fake = rel(fake_pred, real_pred.detach(), fake, is_disc) / 2, backward
    then opt_d.step().  These are five forwards of D: in train mode one step advances every u and v of a spectral-norm D by
    five power iterations, as the published loop does.

    `disc`: any module of fp32 NCHW in, logits (of any shape) out; it is left in the mode it came in.  Returns (l_pix,
    l_percep, l_g_gan, l_d_real, l_d_fake, fake) as detached device tensors: the unweighted L1, the (weighted) content term
    (a zero scalar without vggfeat), the generator's GAN term and D's two terms with their 1/2 inside, as BasicSR logs them.
    One stream, no host read: usable inside GraphedStep with a FusedAdam for each optimiser."""
    rel = F.relativistic_gan_loss
    d_params = [p for p in disc.parameters()]
    # --- generator
    with _requires_grad(d_params, False):
        opt_g.zero_grad()
        fake = gen(lq)
        l_pix = F.l1_loss(fake, gt)
        l_g = F.scale_loss(l_pix, float(l1_weight))
        if vggfeat is not None:
            l_percep = vggfeat(fake, gt)
            l_g = F.add_losses(l_g, l_percep)
        else:
            l_percep = torch.zeros((), dtype=torch.float32, device=fake.device)
        with torch.no_grad():
            real_pred = disc(gt)
        fake_pred = disc(fake)
        l_g_gan = F.scale_loss(F.add_losses(rel(real_pred, fake_pred, False, gan_type, is_disc=False),
                                            rel(fake_pred, real_pred, True, gan_type, is_disc=False)), 0.5)
        l_g = F.add_losses(l_g, F.scale_loss(l_g_gan, float(gan_weight)))
        with F.batched_wgrad():
            l_g.backward()
        opt_g.step()
        if ema is not None:
            ema.update()
    # --- discriminator
    with _requires_grad(d_params, True):
        opt_d.zero_grad()
        fake_det = fake.detach()
        with torch.no_grad():
            fake_pred = disc(fake_det)
        real_pred = disc(gt)
        l_d_real = F.scale_loss(rel(real_pred, fake_pred, True, gan_type, is_disc=True), 0.5)
        with F.batched_wgrad():
            l_d_real.backward()
        fake_pred = disc(fake_det)
        l_d_fake = F.scale_loss(rel(fake_pred, real_pred.detach(), False, gan_type, is_disc=True), 0.5)
        with F.batched_wgrad():
            l_d_fake.backward()
        opt_d.step()
    return l_pix.detach(), l_percep.detach(), l_g_gan.detach(), l_d_real.detach(), l_d_fake.detach(), fake_det


class GraphedStep:
    """A whole step (forward, backward, fused Adam) captured once in a HIP graph and replayed.

    The small workloads are launch-bound (config 2: ~500 kernel launches for 8 ms of work; a DIP iteration likewise), and
    everything a step does is capturable by construction: the C ABI only enqueues on the given stream, never
    allocates or synchronises, the Adam step counter and the BatchNorm batch counters live on the device, and
    scratch comes from torch's allocator (graph-private pool during capture).  `fn` must read its inputs from fixed
    tensors and return tensors; the returned tensors are the graph's static outputs (overwritten by each replay)."""

    def __init__(self, fn, warmup=3):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                    # warm-up off the default stream, as graph capture requires
            for _ in range(warmup):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = fn()

    def __call__(self):
        self.graph.replay()
        return self.out


class DipRunner:
    """DIP.py:22-123 state: fixed noise input, jitter buffer, Lanczos downsampler, Adam over the net."""

    def __init__(self, net, downsampler, net_input, lr_image, learning_rate, reg_noise_std, loss_scale=None,
                 max_grad_norm=None, learn_downsampler=False):
        from .optim import DynamicLossScaler, FusedAdam
        # fp16 storage (the DIP default, see models/DIP/skip.py) needs a loss scale so that activation
        # gradients (~1e-5 at the MSE) stay out of fp16's subnormal range; Adam un-scales on the fly.
        # None: static 1024 (tuned at HR 128x128, x2); a number: that static scale; "dynamic" or an
        # optim.DynamicLossScaler: the scale follows the gradients on the device, overflowing steps are skipped.
        # max_grad_norm: FusedAdam's device-side clipping of the global gradient norm (of the un-scaled gradients).
        self.scaler = None
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError(f"loss_scale: a number, None, 'dynamic' or a DynamicLossScaler, got {loss_scale!r}")
            loss_scale = DynamicLossScaler()
        if isinstance(loss_scale, DynamicLossScaler):
            self.scaler, loss_scale = loss_scale, 1.0
        elif loss_scale is None:
            loss_scale = 1024.0 if getattr(net, "compute_dtype", None) == torch.float16 else 1.0
        self.loss_scale = float(loss_scale)
        self.net, self.down = net, downsampler
        self.net_input_saved = net_input.detach().clone()        # DIP.py:33
        self.noise = net_input.detach().clone()                  # DIP.py:34
        self.net_input = net_input
        self.lr_image = lr_image
        self.sigma = reg_noise_std
        params = list(net.parameters())                          # get_params('net')
        if learn_downsampler:
            # blind super-resolution: the downsampler's weight and bias join the same Adam (and its loss scale / clipping)
            if not hasattr(downsampler, "set_learnable"):
                raise TypeError(f"learn_downsampler=True needs a downsampler with trainable filters (utils.downsampler."
                                f"Downsampler); {type(downsampler).__name__} has no set_learnable()")
            downsampler.set_learnable(True)
            params = params + list(downsampler.parameters())
        self.opt = FusedAdam(params, lr=learning_rate, grad_scale=1.0 / self.loss_scale,
                             max_grad_norm=max_grad_norm)            # utils/DIP.py:34

    def step(self, noise=None):
        """optimizer.zero_grad(); closure(); optimizer.step()  (utils/DIP.py:35-38, DIP.py:47-68)."""
        self.opt.zero_grad()
        if self.sigma > 0:
            if noise is None:
                noise = self.noise.normal_()                     # DIP.py:52 (torch RNG on whatever device holds it)
            self.net_input = self.net_input_saved + noise * self.sigma
        out_hr = self.net(self.net_input)                        # :60
        out_lr = self.down(out_hr)                               # :62
        loss = F.mse_loss(out_lr, self.lr_image)                 # :65
        if self.scaler is not None:
            _backward_and_step(loss, self.opt, self.scaler)      # :68 under the dynamic scale
            return loss.detach(), out_hr.detach()
        with F.batched_wgrad():
            F.scale_loss(loss, self.loss_scale).backward()       # :68
        self.opt.step()
        return loss.detach(), out_hr.detach()
