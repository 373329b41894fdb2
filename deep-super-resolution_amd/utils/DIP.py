"""Deep-Image-Prior optimisation helpers behind the reference's surface (/root/reference/utils/DIP.py:7-105):
``optimize``, ``get_params``, ``fill_noise``, ``get_noise`` -- same names, argument meaning and error behaviour
(bare ``assert`` on an unknown option), written around this package's fused HIP Adam.

Host-side glue: the closure the caller passes in runs the HIP network; nothing here touches activations."""
import numpy as np
import torch

from ..functional import batched_wgrad
from ..optim import DynamicLossScaler, FusedAdam, FusedLBFGS

# utils/DIP.py:21 -- the LBFGS branch first takes 100 Adam steps at this fixed rate
LBFGS_WARMUP_STEPS = 100
LBFGS_WARMUP_LR = 0.001


def _scaler(loss_scale):
    """None, or the DynamicLossScaler that ``loss_scale`` ("dynamic" or an instance) stands for."""
    if loss_scale is None or isinstance(loss_scale, DynamicLossScaler):
        return loss_scale
    if loss_scale == "dynamic":
        return DynamicLossScaler()
    raise ValueError(f"loss_scale: None, 'dynamic' or an optim.DynamicLossScaler, got {loss_scale!r}")


def _adam_loop(parameters, closure, learning_rate, steps, scaler=None, max_grad_norm=None):
    """zero_grad(); closure(); step()  `steps` times with the fused multi-tensor Adam kernel (utils/DIP.py:33-38).

    ``scaler``: the closure calls backward() itself on a loss this function never sees, so the scale is applied where the
    fp32 gradient enters the net's 16-bit storage (functional.ambient_loss_scale) -- the same numbers as a scaled loss.
    On that route the closure's 3x3 weight gradients are also grouped into one launch as steps.DipRunner groups them
    (functional.batched_wgrad: nothing in the closure may read a weight's .grad), so the two routes give the same bits; the
    route without a scaler keeps its launches, and its bits, as they were.  ``max_grad_norm``: FusedAdam's device-side
    clipping of the global gradient norm."""
    optimizer = FusedAdam(parameters, lr=learning_rate, max_grad_norm=max_grad_norm)
    for _ in range(steps):
        optimizer.zero_grad()
        if scaler is None:
            closure()
            optimizer.step()
        else:
            with scaler.ambient(parameters[0].device), batched_wgrad():
                closure()
            scaler.step(optimizer)
            scaler.update()
    optimizer.zero_grad(set_to_none=True)


def _lbfgs(parameters, closure, learning_rate, num_iter, fused=False, scaler=None, max_grad_norm=None):
    """utils/DIP.py:19-31: Adam warm-up, then ONE torch.optim.LBFGS.step of ``max_iter=num_iter`` inner iterations
    with both tolerances disabled.  The closure (forward, loss, backward) is the HIP path; by default the two-loop
    recursion itself is torch's own vector arithmetic on the flattened parameters, exactly as in the reference.  LBFGS
    writes the parameters in place through torch ops, which bumps their version counters, so the packed 16-bit weight
    images are refreshed on the next forward.  ``fused``: the same step by ``optim.FusedLBFGS`` (csrc/lbfgs.hip), which
    refreshes those images itself after each update.  ``scaler`` and ``max_grad_norm`` serve the Adam warm-up only."""
    parameters = list(parameters)
    _adam_loop(parameters, closure, LBFGS_WARMUP_LR, LBFGS_WARMUP_STEPS, scaler, max_grad_norm)
    cls = FusedLBFGS if fused else torch.optim.LBFGS
    optimizer = cls(parameters, max_iter=num_iter, lr=learning_rate, tolerance_grad=-1, tolerance_change=-1)

    def closure2():
        optimizer.zero_grad()
        return closure()

    optimizer.step(closure2)


def optimize(optimizer_type, parameters, closure, learning_rate, num_iter, *, fused_lbfgs=False, loss_scale=None,
             max_grad_norm=None):
    """Run the optimisation loop: ``'adam'`` (what DIP.py:99 selects) or ``'LBFGS'``; anything else asserts.
    ``fused_lbfgs=True`` runs the LBFGS branch's L-BFGS phase on ``optim.FusedLBFGS`` instead of torch.optim.LBFGS.

    ``loss_scale="dynamic"`` (or an ``optim.DynamicLossScaler``): the fp16 net's gradients are computed under a loss scale
    that follows them on the device; steps whose gradients overflow are skipped.  The closure stays as it is.  Without it
    the gradients are unscaled, as before.  With ``'LBFGS'`` it applies to the 100-step Adam warm-up only: the L-BFGS phase
    takes no loss scale (closure values and curvature pairs do not survive skipped steps).

    ``max_grad_norm=c``: the Adam steps clip the global 2-norm of the gradients to ``c`` on the device
    (``optim.FusedAdam(max_grad_norm=c)``); with ``'LBFGS'`` that is the warm-up only, FusedLBFGS takes no clipping."""
    scaler = _scaler(loss_scale)
    runners = {'adam': lambda: _adam_loop(list(parameters), closure, learning_rate, num_iter, scaler, max_grad_norm),
               'LBFGS': lambda: _lbfgs(parameters, closure, learning_rate, num_iter, fused=fused_lbfgs, scaler=scaler,
                                       max_grad_norm=max_grad_norm)}
    assert optimizer_type in runners
    runners[optimizer_type]()


def get_params(opt_over, net, net_input, downsampler=None):
    """Tensors to optimise over for a comma-separated ``opt_over`` of 'net', 'down', 'input' (utils/DIP.py:44-68).

    Bug-compatible with the reference on one point: 'down' REPLACES whatever was collected before it instead of
    extending it (utils/DIP.py:61 assigns), so "net,down" yields the downsampler's parameters only.  'down' also
    switches a utils.downsampler.Downsampler to its dense, differentiable forward (``set_learnable(True)``)."""
    params = []
    for what in opt_over.split(','):
        if what == 'net':
            params = params + list(net.parameters())
        elif what == 'down':
            assert downsampler is not None
            if hasattr(downsampler, 'set_learnable'):
                downsampler.set_learnable(True)       # forward through the dense op: these parameters get gradients
            params = list(downsampler.parameters())
        elif what == 'input':
            net_input.requires_grad = True
            params = params + [net_input]
        else:
            assert False, 'what is it?'
    return params


_FILLERS = {'u': torch.Tensor.uniform_, 'n': torch.Tensor.normal_}


def fill_noise(x, noise_type):
    """In-place U(0,1) ('u') or N(0,1) ('n') from torch's generator of x's device (utils/DIP.py:70-77)."""
    assert noise_type in _FILLERS
    _FILLERS[noise_type](x)


def get_noise(input_depth, method, spatial_size, noise_type='u', var=1. / 10):
    """[1, input_depth, H, W] network input (utils/DIP.py:79-105): 'noise' = noise * var drawn on the CPU default
    generator like the reference (DIP.py:32 then moves it to the device), 'meshgrid' = the two normalised coordinate
    planes (float64, x first), which needs input_depth == 2."""
    h, w = (spatial_size, spatial_size) if isinstance(spatial_size, int) else spatial_size[:2]
    if method == 'noise':
        net_input = torch.zeros([1, input_depth, h, w])
        fill_noise(net_input, noise_type)
        return net_input.mul_(var)
    if method == 'meshgrid':
        assert input_depth == 2
        xs, ys = np.meshgrid(np.arange(0, w) / float(w - 1), np.arange(0, h) / float(h - 1))
        return torch.from_numpy(np.stack([xs, ys]))[None]
    assert False
