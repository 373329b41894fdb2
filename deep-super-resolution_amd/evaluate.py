"""Checkpoint interchange and the generator evaluation loop on the HIP path.

Counterparts of the reference's host glue, kept format-compatible so that ``.pth`` files move both ways:
  save_model / load_model      utils/common.py:11-18, 46-60  (``torch.save(model.state_dict())``; ``module.`` prefix of a
                               DataParallel/DDP-wrapped model stripped on load)
  evaluate_generator           eval_GAN.py:21-69  (``gan_G.eval()``, one image at a time, PSNR average, PNG dump) --
                               run under ``no_grad`` and optionally halo-tiled (infer.super_resolve), which the reference's
                               loop lacks (its images are pre-shrunk "because too big for the forward pass", dataset.py:21-23)

PSNR is 10*log10(range^2 / MSE) (torchmetrics' definition; that package is absent here, so the formula is restated --
"parity unpinned").  ``data_range=None`` infers max-min of the target like ``PeakSignalNoiseRatio()`` does.
The MSE is reduced on the device by the HIP loss kernel; only the final scalar crosses to the host.
LPIPS is ``lpips.LPIPS`` (AlexNet trunk on the HIP path); ``lpips()`` below is the reference's helper around it.
"""
import math
import os
from collections import OrderedDict

import torch

from . import functional as F
from . import infer


def save_model(model, name, out_dir):
    """utils/common.py:11-18: <out_dir>/<name>.pth holding model.state_dict() (tensors moved to the host so that the file
    loads anywhere)."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.pth")
    torch.save(OrderedDict((k, v.detach().cpu()) for k, v in model.state_dict().items()), path)
    return path


def load_model(model, model_path):
    """utils/common.py:46-60: load a reference-format checkpoint, with or without the ``module.`` key prefix.
    ``weights_only=True`` (as in the reference): nothing in the file is executed.  A file that wraps the state dict as
    ``{'params_ema': ...}`` or ``{'params': ...}`` (BasicSR's format: models/GAN/rrdbnet.py) is unwrapped, the average first."""
    state = torch.load(model_path, map_location="cpu", weights_only=True)
    for key in ("params_ema", "params"):     # BasicSR's wrapping (ESRGAN / Real-ESRGAN checkpoints); it prefers the average too
        if isinstance(state.get(key), dict):
            state = state[key]
            break
    clean = OrderedDict((k[len("module."):] if k.startswith("module.") else k, v) for k, v in state.items())
    model.load_state_dict(clean)
    return model


def interpolate_state_dicts(sd_a, sd_b, alpha):
    """ESRGAN's network interpolation (net_interp.py): a state dict between the PSNR-trained generator `sd_a` and the
    GAN-trained one `sd_b`.  Every floating tensor becomes (1 - alpha) * a + alpha * b, computed in fp32 and cast back to a's
    dtype; every other entry (an integer buffer such as a batch counter) is taken from `sd_b`.  The two dicts must hold the
    same keys with the same shapes: anything else is a ValueError that names the key.  Plain torch on whatever device the
    tensors live on; the result loads into a fresh RRDBNet / Generator."""
    alpha = float(alpha)
    only = [k for k in sd_a if k not in sd_b] + [k for k in sd_b if k not in sd_a]
    if only:
        raise ValueError(f"interpolate_state_dicts: key {only[0]!r} is in one state dict only ({len(only)} such keys)")
    out = OrderedDict()
    for k, a in sd_a.items():
        b = sd_b[k]
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"interpolate_state_dicts: {k!r} has shape {tuple(a.shape)} in one state dict and {tuple(b.shape)} "
                             "in the other")
        if a.is_floating_point() and b.is_floating_point():
            out[k] = (a.detach().float() * (1.0 - alpha) + b.detach().float() * alpha).to(a.dtype)
        else:
            out[k] = b.detach().clone()
    return out


def vgg_discriminator_layout(num_in_ch=3, num_feat=64, input_size=128):
    """[(key, shape)] of the state dict of BasicSR's ``VGGStyleDiscriminator(num_in_ch, num_feat, input_size)``, in torch's
    order: the ``net_d`` checkpoints that go with the ESRGAN generators.  conv0_0 (3x3, bias), then per stage conv{s}_1 / bn{s}_1
    (4x4 stride 2) behind conv{s}_0 / bn{s}_0 (3x3), no conv bias, widths nf | 2nf | 4nf | 8nf | 8nf (| 8nf for input_size
    256), linear1 (8nf * 4 * 4 -> 100), linear2 (100 -> 1).  The module itself is not in this package yet; this is its
    checkpoint surface, written from the published definition (parity with BasicSR unpinned; tests/test_host_vggd.py holds
    it to a copy built from torch.nn layers)."""
    if input_size not in (128, 256):
        raise ValueError(f"vgg_discriminator_layout: input_size must be 128 or 256, got {input_size}")
    nf = int(num_feat)
    if nf < 1 or int(num_in_ch) < 1:
        raise ValueError(f"vgg_discriminator_layout: num_in_ch and num_feat must be positive, got {num_in_ch}, {num_feat}")
    out = [("conv0_0.weight", (nf, int(num_in_ch), 3, 3)), ("conv0_0.bias", (nf,))]

    def block(conv, bn, cout, cin, k):
        return [(conv + ".weight", (cout, cin, k, k)), (bn + ".weight", (cout,)), (bn + ".bias", (cout,)),
                (bn + ".running_mean", (cout,)), (bn + ".running_var", (cout,)), (bn + ".num_batches_tracked", ())]

    out += block("conv0_1", "bn0_1", nf, nf, 4)
    widths = [(nf, 2 * nf), (2 * nf, 4 * nf), (4 * nf, 8 * nf), (8 * nf, 8 * nf)] + ([(8 * nf, 8 * nf)] if input_size == 256 else [])
    for s, (cin, cout) in enumerate(widths, start=1):
        out += block(f"conv{s}_0", f"bn{s}_0", cout, cin, 3) + block(f"conv{s}_1", f"bn{s}_1", cout, cout, 4)
    return out + [("linear1.weight", (100, 8 * nf * 16)), ("linear1.bias", (100,)), ("linear2.weight", (1, 100)),
                  ("linear2.bias", (1,))]


def inspect_vgg_discriminator(state):
    """{'num_in_ch', 'num_feat', 'input_size', 'parameters'} of a ``VGGStyleDiscriminator`` state dict, read off conv0_0's
    shape and the presence of stage 5, after checking every key and shape against vgg_discriminator_layout.  `state` may carry
    BasicSR's ``{'params': ...}`` / ``{'params_ema': ...}`` wrapping and the ``module.`` prefix, as load_model accepts them.  A
    missing, unexpected or misshapen entry is a ValueError that names the key.  Plain torch, offline."""
    for key in ("params_ema", "params"):
        if isinstance(state.get(key), dict):
            state = state[key]
            break
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    w0 = sd.get("conv0_0.weight")
    if w0 is None or w0.dim() != 4:
        raise ValueError("inspect_vgg_discriminator: 'conv0_0.weight' is missing or not a 4-d tensor")
    nf, cin = int(w0.shape[0]), int(w0.shape[1])
    size = 256 if "conv5_0.weight" in sd else 128
    layout = vgg_discriminator_layout(cin, nf, size)
    want = dict(layout)
    extra = [k for k in sd if k not in want]
    if extra:
        raise ValueError(f"inspect_vgg_discriminator: unexpected key {extra[0]!r} ({len(extra)} such keys)")
    for k, shape in layout:
        if k not in sd:
            raise ValueError(f"inspect_vgg_discriminator: key {k!r} is missing")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"inspect_vgg_discriminator: {k!r} has shape {tuple(sd[k].shape)}, expected {shape} for "
                             f"num_in_ch={cin}, num_feat={nf}, input_size={size}")
    params = sum(math.prod(shape) for k, shape in layout if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    return {"num_in_ch": cin, "num_feat": nf, "input_size": size, "parameters": params}


def inspect_srvgg(state):
    """dict(num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type): the constructor arguments of the
    ``models.GAN.srvgg.SRVGGNetCompact`` that a checkpoint loads into, read off its keys and shapes.  `state` may be plain,
    carry BasicSR's ``{'params_ema': ...}`` / ``{'params': ...}`` wrapping, and the ``module.`` prefix, as load_model accepts
    them.  num_out_ch is num_in_ch (the network adds its input to its output) and upscale = sqrt(Cout_last / num_in_ch) must
    be an integer.  act_type is 'prelu' when the odd-index keys ``body.{odd}.weight`` exist, else None: ReLU and LeakyReLU
    have no parameters, so a file cannot tell them apart.  A missing, unexpected or misshapen key is a ValueError that names
    the key.  Plain torch, offline."""
    for key in ("params_ema", "params"):
        if isinstance(state.get(key), dict):
            state = state[key]
            break
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    idx = {}
    for k in sd:
        parts = k.split(".")
        if len(parts) != 3 or parts[0] != "body" or not parts[1].isdigit() or parts[2] not in ("weight", "bias"):
            raise ValueError(f"inspect_srvgg: unexpected key {k!r}")
        idx.setdefault(int(parts[1]), set()).add(parts[2])
    w0 = sd.get("body.0.weight")
    if w0 is None or w0.dim() != 4:
        raise ValueError("inspect_srvgg: 'body.0.weight' is missing or not a 4-d tensor")
    nf, cin = int(w0.shape[0]), int(w0.shape[1])
    last = max(i for i in idx if i % 2 == 0)
    if last < 2:
        raise ValueError("inspect_srvgg: key 'body.2.weight' is missing (the network has a head and a tail at least)")
    num_conv = (last - 2) // 2
    prelu = any(i % 2 for i in idx)
    want = OrderedDict()
    for i in range(0, last + 1, 2):
        want[f"body.{i}.weight"] = (nf if i < last else None, cin if i == 0 else nf, 3, 3)
        want[f"body.{i}.bias"] = (nf if i < last else None,)
        if prelu and i < last:
            want[f"body.{i + 1}.weight"] = (nf,)
    for k in sd:
        if k not in want:
            raise ValueError(f"inspect_srvgg: unexpected key {k!r}")
    for k, shape in want.items():
        if k not in sd:
            raise ValueError(f"inspect_srvgg: key {k!r} is missing")
        got = tuple(sd[k].shape)
        if len(got) != len(shape) or any(s is not None and s != g for s, g in zip(shape, got)):
            raise ValueError(f"inspect_srvgg: {k!r} has shape {got}, expected {shape} for num_in_ch={cin}, num_feat={nf}")
    q = int(sd[f"body.{last}.weight"].shape[0])
    s = math.isqrt(q // cin) if q % cin == 0 else 0
    if s < 1 or s * s * cin != q:
        raise ValueError(f"inspect_srvgg: 'body.{last}.weight' has {q} outputs, which is not num_in_ch ({cin}) times a square")
    if tuple(sd[f"body.{last}.bias"].shape) != (q,):
        raise ValueError(f"inspect_srvgg: 'body.{last}.bias' has shape {tuple(sd[f'body.{last}.bias'].shape)}, expected {(q,)}")
    return dict(num_in_ch=cin, num_out_ch=cin, num_feat=nf, num_conv=num_conv, upscale=s, act_type="prelu" if prelu else None)


def psnr(pred, target, data_range=None):
    """Host float: 10*log10(range^2 / MSE(pred, target)) for fp32 NCHW device tensors.
    ``data_range=None`` follows what torchmetrics' ``PeakSignalNoiseRatio()`` (eval_GAN.py:30,47: the metric is CALLED per
    image, which evaluates that image from the metric's default state) does as far as its published behaviour goes: the range
    is max(target.max(), 0) - min(target.min(), 0) -- its running minimum and maximum start at 0, so a [0.2, 0.9] target has
    range 0.9, not 0.7.  torchmetrics is absent from /root/reference and from this image: PARITY UNPINNED."""
    mse = float(F.mse_loss(pred.detach(), target.detach()))
    if data_range is None:
        data_range = max(float(target.max()), 0.0) - min(float(target.min()), 0.0)
    return 10.0 * math.log10(data_range ** 2 / mse) if mse > 0 else float("inf")


def ssim(pred, target, data_range=1.0):
    """Host float: mean SSIM (Gaussian 11x11, sigma 1.5, K1 0.01, K2 0.03 -- the torchmetrics defaults the reference's scripts
    run with, ``SSIM(data_range=1.)`` at eval_GAN.py:31) of fp32 NCHW device tensors, on the HIP kernel dsr_ssim_img_f32: the
    value of ``metrics.SSIM(data_range=data_range)(pred, target)``, bit for bit."""
    from . import metrics
    pred, target = pred.detach().contiguous().float(), target.detach().contiguous().float()
    if pred.shape != target.shape or pred.dim() != 4 or pred.numel() == 0:
        raise RuntimeError(f"ssim: operands must be two [N,C,H,W] tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    n, _, h, w = pred.shape
    if h < 11 or w < 11:
        raise RuntimeError(f"ssim: images of {h}x{w} are smaller than the 11x11 window")
    if not data_range > 0:
        raise RuntimeError(f"ssim: data_range must be positive, got {data_range!r}")
    _, total = metrics._ssim_img("ssim", pred, target, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, 1.0 / n)
    return float(total)


def lpips(im0, im1, lpips_model):
    """utils/common.py:105-109: host float of ``lpips_model(im0, im1)`` under ``no_grad`` (an ``lpips.LPIPS``)."""
    with torch.no_grad():
        return float(lpips_model(im0, im1))


def to_uint8_image(img):
    """[3,H,W] float in [0,1] -> [H,W,3] uint8 numpy (eval_GAN.py:55-56; values are clipped first, the reference's bare
    ``astype(np.uint8)`` wraps out-of-range values)."""
    return (img.detach().clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()


def bicubic_pairs(hr_images, scale):
    """The benchmark protocol's test pairs from HR images alone: each uint8 [H, W, 3] image (device tensor, numpy array or PIL
    image; or an ``(image, name)`` pair -- the default name is the image's position) is cropped to a multiple of `scale`
    (``modcrop``) and reduced by the MATLAB-style ``utils.imresize.imresize(hr, 1 / scale)`` to its 8-bit LR image, on the
    device.  Returns a list of ``(LR [1,3,h,w], HR [1,3,H,W], name)`` fp32 in [0, 1]: what ``evaluate_generator`` takes; with
    ``y_channel=True`` its 'psnr_y' / 'ssim_y' then follow the published tables end to end on the device (MATLAB's own uint8
    rounding between the two resampling passes is unpinned, see utils/imresize.py)."""
    from .dataset import to_tensor
    from .utils.degradation import _to_device
    from .utils.imresize import imresize, modcrop
    out = []
    for i, item in enumerate(hr_images):
        image, name = item if isinstance(item, (tuple, list)) else (item, str(i))
        hr = modcrop(_to_device(image)[0], scale).contiguous()
        lr = imresize(hr, scale=1.0 / scale)
        out.append((to_tensor(lr)[None], to_tensor(hr)[None], name))
    return out


def evaluate_generator(gen, pairs, tile=None, out_dir=None, data_range=None, dtype=torch.float16, to_unit=None,
                       with_ssim=True, lpips_model=None, self_ensemble=False, ema=None, y_channel=False, shave=None,
                       niqe_model=None):
    """eval_GAN.py:21-69 for an iterable of (LR [1,3,h,w], HR [1,3,H,W], name) on the device.

    Returns {'avg_psnr': ..., 'psnr': {name: value}, 'avg_ssim': ..., 'ssim': {name: value}}, and with ``lpips_model`` (an
    ``lpips.LPIPS``; eval_GAN.py:32,49) also 'avg_lpips' (the reference's key, :66) and 'lpips': {name: value}; its numbers
    are the trained metric's only when the model was given the AlexNet and head weights.  ``out_dir`` (optional) receives <out_dir>/images/<name>.png like
    save_image (utils/common.py:20-33); ``to_unit`` maps the network's output range to [0,1] for the PNG (default:
    identity, as in the reference).  ``self_ensemble`` (True, or a sequence of D4 codes) scores the geometric self-ensemble
    of ``infer.super_resolve`` instead of the single forward.  ``ema`` (an ``optim.WeightEMA`` over ``gen``) scores the
    averaged weights: they are swapped into ``gen`` for the loop and out again afterwards, also when the loop raises.

    ``y_channel=True`` adds the numbers of the published super-resolution tables next to the ones above, which stay as they
    are: 'avg_psnr_y', 'psnr_y' and (with ``with_ssim``) 'avg_ssim_y', 'ssim_y' -- PSNR and SSIM of the BT.601 luma of the
    8-bit-quantised output against that of the target, ``shave`` pixels cut from each border (``metrics.PSNR_Y`` /
    ``metrics.SSIM_Y``; the images are taken to be in [0, 1]).  ``shave=None`` is the scale factor, HR height // LR height.
    That path reads nothing on the host inside the loop: the per-image values stay on the device and cross once at the end.

    ``niqe_model`` (a ``metrics.NaturalnessImageQualityEvaluator``) adds 'avg_niqe' and 'niqe': {name: value}, the no-reference
    score of each super-resolved image (the target is not looked at; images too small for two 96 x 96 blocks are a ValueError).
    The block statistics stay on the device inside the loop and cross once at the end."""
    if niqe_model is not None and not (hasattr(niqe_model, "statistics") and hasattr(niqe_model, "mu_p")):
        raise TypeError(f"evaluate_generator: niqe_model must be a metrics.NaturalnessImageQualityEvaluator, got "
                        f"{type(niqe_model).__name__}")
    if ema is not None:
        if ema.module is not gen:
            raise ValueError("evaluate_generator: `ema` averages another module than `gen`")
        with ema.average_parameters():
            return evaluate_generator(gen, pairs, tile=tile, out_dir=out_dir, data_range=data_range, dtype=dtype,
                                      to_unit=to_unit, with_ssim=with_ssim, lpips_model=lpips_model,
                                      self_ensemble=self_ensemble, y_channel=y_channel, shave=shave, niqe_model=niqe_model)
    if shave is not None and (isinstance(shave, bool) or not isinstance(shave, int) or shave < 0):
        raise ValueError(f"evaluate_generator: shave must be None or a non-negative integer, got {shave!r}")
    per, ssims, lps = OrderedDict(), OrderedDict(), OrderedDict()
    y_names, y_psnr, y_ssim = [], [], []                    # device tensors, one [1] per image
    q_names, q_stats = [], []                               # NIQE: device statistics, one [1, 1333] per image
    for lr_image, hr_image, name in pairs:
        if isinstance(name, (list, tuple)):
            name = name[0]                                  # DataLoader collation of a batch of one (eval_GAN.py:40)
        resolved = infer.super_resolve(gen, lr_image, tile=tile, dtype=dtype, self_ensemble=self_ensemble)
        per[name] = psnr(resolved, hr_image, data_range)
        if with_ssim:
            ssims[name] = ssim(resolved, hr_image, 1.0)          # SSIM(data_range=1.) as at eval_GAN.py:31
        if lpips_model is not None:
            lps[name] = lpips(resolved, hr_image, lpips_model)   # eval_GAN.py:49
        if y_channel:
            from . import metrics
            border = hr_image.shape[2] // lr_image.shape[2] if shave is None else shave
            p_y, s_y = metrics.luma_psnr_ssim(resolved, hr_image, shave=border, quantize=True, with_ssim=with_ssim)
            y_names.append(name)
            y_psnr.append(p_y)
            y_ssim.append(s_y)
        if niqe_model is not None:
            q_names.append(name)
            q_stats.append(niqe_model.statistics(resolved))
        if out_dir is not None:
            from PIL import Image
            img_dir = os.path.join(out_dir, "images")
            os.makedirs(img_dir, exist_ok=True)
            img = resolved[0] if to_unit is None else to_unit(resolved[0])
            Image.fromarray(to_uint8_image(img)).save(os.path.join(img_dir, f"{name}.png"))
    out = {"avg_psnr": sum(per.values()) / max(len(per), 1), "psnr": per}
    if with_ssim:
        out.update(avg_ssim=sum(ssims.values()) / max(len(ssims), 1), ssim=ssims)
    if lpips_model is not None:
        out.update(avg_lpips=sum(lps.values()) / max(len(lps), 1), lpips=lps)
    if y_channel:
        cols = [y_psnr, y_ssim] if with_ssim else [y_psnr]
        host = torch.stack([torch.cat(c) for c in cols]).double().cpu().tolist() if y_names else [[] for _ in cols]
        for key, vals in zip(("psnr_y", "ssim_y"), host):
            out["avg_" + key] = sum(vals) / max(len(vals), 1)
            out[key] = OrderedDict(zip(y_names, vals))
    if niqe_model is not None:
        vals = _niqe_values(niqe_model, q_stats)
        out.update(avg_niqe=sum(vals) / max(len(vals), 1), niqe=OrderedDict(zip(q_names, vals)))
    return out


def _niqe_values(niqe_model, stats):
    """Host floats, one per image, from a list of device statistics: one transfer."""
    if not stats:
        return []
    from . import metrics
    return metrics.niqe_score(torch.cat(stats).cpu().numpy(), niqe_model.mu_p, niqe_model.cov_p).tolist()


def score_niqe(gen, lr_images, niqe_model, **super_resolve_kwargs):
    """NIQE of the super-resolved images of LR inputs that have no HR counterpart -- the real-world protocol of Real-ESRGAN.

    ``lr_images``: an iterable of [N, 3, h, w] device tensors in [0, 1], or of ``(tensor, name)`` pairs (the default name is the
    position; an image of a batch N > 1 is named ``<name>/<i>``).  ``niqe_model``: a ``metrics.NaturalnessImageQualityEvaluator``.
    The keyword arguments go to ``infer.super_resolve`` (``tile``, ``halo``, ``dtype``, ``self_ensemble``, ``ensemble_batch``).
    Returns {'avg_niqe': ..., 'niqe': {name: value}}; the statistics cross to the host once, after the loop."""
    if not (hasattr(niqe_model, "statistics") and hasattr(niqe_model, "mu_p")):
        raise TypeError(f"score_niqe: niqe_model must be a metrics.NaturalnessImageQualityEvaluator, got "
                        f"{type(niqe_model).__name__}")
    names, stats = [], []
    for i, item in enumerate(lr_images):
        lr, name = item if isinstance(item, (tuple, list)) else (item, str(i))
        resolved = infer.super_resolve(gen, lr, **super_resolve_kwargs)
        stats.append(niqe_model.statistics(resolved))
        n = resolved.shape[0]
        names += [name] if n == 1 else [f"{name}/{k}" for k in range(n)]
    vals = _niqe_values(niqe_model, stats)
    return {"avg_niqe": sum(vals) / max(len(vals), 1), "niqe": OrderedDict(zip(names, vals))}
