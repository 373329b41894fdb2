"""Adam with torch.optim.Adam's default semantics (train_GAN.py:35-36, utils/DIP.py:34) as one fused
HIP kernel per tensor; the step counter lives on the device so a whole train step can be captured
in a HIP graph.  L-BFGS with torch.optim.LBFGS's semantics (utils/DIP.py:24-31) as four HIP passes
per closure call, its whole state on the device.  WeightEMA: torch.optim.swa_utils.AveragedModel's exponential
moving average of a model's weights, one multi-tensor HIP launch per 64 tensors, its counter on the device."""
import contextlib
import ctypes as C
import math
from collections import OrderedDict

import torch

from . import _lib
from ._lib import ptr_table, size_table
from .functional import _need_gpu, _ptr, _stream, bump, check, mark_shadow_current, repack_cached, shadow_for_update


class FusedAdam:
    MULTI_MAX = 1 << 20      # tensors up to this many elements go through the multi-tensor launch

    GRAM_MAX_ROWS = 512      # ranks x padded batch up to which the factored gradient's norm comes from the Gram identity

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, fuse_dense_head=False,
                 max_grad_norm=None, norm_type=2.0):
        """``lr``: a float, or a one-element tensor (torch.optim.Adam's capturable form): cast to fp32 on the parameters'
        device and kept as ``self.lr``; every Adam launch reads it on the device, so ``opt.lr.fill_(x)`` takes effect at the
        next ``step()`` and at the next replay of a captured step (steps.GraphedStep).  A tensor holding the fp32 value of a
        float gives that float's bits.

        ``max_grad_norm=c``: ``torch.nn.utils.clip_grad_norm_(params, c, norm_type=2.0, error_if_nonfinite=False)`` followed
        by Adam, on the device: ``step()`` forms the global 2-norm over every parameter of this optimiser that has a gradient
        -- the dense head's deferred gradient included, from its two factors, which torch's function cannot see -- and the
        Adam kernels apply ``clip_coef = min(1, c / (grad_norm + 1e-6))``.  The gradients themselves are NOT rewritten:
        ``p.grad`` after ``step()`` holds the unclipped gradient.  ``self.grad_norm`` / ``self.clip_coef`` (fp32 device
        tensors [1]) hold this step's norm of the TRUE gradient -- a static ``grad_scale`` and a DynamicLossScaler's scale
        are taken out -- before clipping, and the coefficient; a non-finite norm gives a NaN coefficient and NaN parameters, as
        in torch.  After a step the scaler skipped they may hold anything, finite or not.  Only the 2-norm is offered.
        With neither option ``step()`` issues the launches it always did."""
        if norm_type is None or isinstance(norm_type, bool) or not isinstance(norm_type, (int, float)) or float(norm_type) != 2.0:
            raise NotImplementedError(f"FusedAdam: norm_type={norm_type!r} is not implemented; only the 2-norm "
                                      "(norm_type=2.0) runs on the HIP path")
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)):
                raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
            if not max_grad_norm > 0:          # (NaN fails the comparison too)
                raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")   # torch.optim raises the same
        dev = self.params[0].device
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError(f"a tensor lr must have one element, got shape {tuple(lr.shape)}")
            self.lr = lr.detach().to(device=dev, dtype=torch.float32).reshape(1)      # (the caller's own storage when it fits)
        else:
            self.lr = float(lr)
        # fuse_dense_head: the dense head's big matrix (discriminator.py:54, marked `_dsr_dense_head`) gets its gradient as
        # two 16-bit factors (functional.GradFactors) instead of a `.grad` tensor, and step() applies Adam inside the
        # weight-gradient contraction (dsr_linear_wgrad_adam).  Same arithmetic, bit for bit; `.grad` of that one tensor
        # stays None, which is why it is opt-in (steps / bench turn it on, nothing else reads that gradient).
        self.fuse_dense_head = bool(fuse_dense_head)
        if self.fuse_dense_head:
            for p in self.params:
                if getattr(p, "_dsr_dense_head", False):
                    p._dsr_defer_wgrad = True
        self.betas, self.eps = betas, float(eps)
        self.grad_scale = float(grad_scale)     # gradients are multiplied by this first (1/S for a loss scale S)
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        # the device hyper block {lr, clip_coef} the Adam kernels read (dsr_adam_args.hyper); dsr_clip_finalize writes it every step
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_coef = torch.ones(1, dtype=torch.float32, device=dev)
        self._hyper = torch.zeros(2, dtype=torch.float32, device=dev)
        self._partials = self._gram_ws = None

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if getattr(p, "_dsr_grad_factors", None):
                p._dsr_grad_factors = []
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _device_hyper(self):
        """True when the Adam launches read lr / the clipping coefficient from the device (dsr_adam_args.hyper)."""
        return self.max_grad_norm is not None or isinstance(self.lr, torch.Tensor)

    def _buffer(self, name, nbytes):
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.step_t.device)
            setattr(self, name, buf)
        return buf

    def _write_hyper(self, grads, factors, scale):
        """The norm pass and dsr_clip_finalize: grad_norm, clip_coef and the hyper block of this step.  `grads`: the fp32
        gradient tensors, `factors`: the deferred GradFactors (already waited for), `scale`: the loss scaler's device word."""
        lib = _lib.lib()
        st = _stream()
        npart, parts, ndots, dots = 0, None, 0, None
        if self.max_grad_norm is not None:
            keep = []
            for f in factors:
                if len(factors) == 1 and f.ranks * f.bp <= self.GRAM_MAX_ROWS:
                    nbytes = lib.dsr_linear_factor_gram_workspace(f.bp, f.o, f.k, f.ranks)
                    ws = self._buffer("_gram_ws", nbytes)
                    check(lib.dsr_linear_factor_gram(f.dt, _ptr(f.dyt), _ptr(f.xt), f.bp, f.o, f.k, f.ranks, f.scale, _ptr(ws),
                                                     nbytes, st))
                    ndots, dots = lib.dsr_linear_factor_gram_dots(f.bp, f.ranks), ws
                else:           # more rows than the Gram kernel takes (or a second factored tensor): the tensor pass
                    keep.append(f.materialize())
            grads = [g for g in list(grads) + keep if g.numel()]
            if grads:
                k = len(grads)
                ptrs, ns = ptr_table(grads), size_table([g.numel() for g in grads])
                npart = lib.dsr_clip_sumsq_partials(k, ptrs, ns)
                parts = self._buffer("_partials", 4 * npart)
                check(lib.dsr_clip_sumsq(k, ptrs, ns, _ptr(parts), npart, st))
        tensor_lr = isinstance(self.lr, torch.Tensor)
        check(lib.dsr_clip_finalize(_ptr(parts), npart, _ptr(dots), ndots, self.grad_scale, _ptr(scale),
                                    self.max_grad_norm or 0.0, _ptr(self.lr) if tensor_lr else None,
                                    0.0 if tensor_lr else self.lr, _ptr(self.grad_norm), _ptr(self.clip_coef),
                                    _ptr(self._hyper), st))

    def step(self, scaler=None):
        """One Adam update.  `scaler` (a DynamicLossScaler whose check of this step's gradients has run; use
        ``scaler.step(optimizer)``): the predicated kernels -- gradients times 1 / scale read on the device, and nothing
        moves, the step counter included, when the scaler's overflow flag is set.  The launch sequence is the same either way.

        With ``max_grad_norm`` or a tensor ``lr`` the Adam launches wait until the norm pass and dsr_clip_finalize have
        written this step's hyper block -- after the overflow check, after a data-parallel run's gradient averaging and the
        dense head's factor gather, so every rank forms the same coefficient -- and read lr and coefficient on the device."""
        lib = _lib.lib()
        st = _stream()
        hyper = self._device_hyper()
        scale = found = None
        if scaler is not None and scaler.enabled:
            if self.grad_scale != 1.0:
                raise ValueError(f"FusedAdam(grad_scale={self.grad_scale}) under a DynamicLossScaler would un-scale the "
                                 "gradients twice: leave grad_scale at 1.0")
            if self.fuse_dense_head:
                raise ValueError("FusedAdam(fuse_dense_head=True) takes no DynamicLossScaler: the dense head's gradient "
                                 "never exists as a tensor that could be checked for overflow, and the bf16 GAN step it "
                                 "serves needs no loss scale")
            scale, found = scaler._state(self.step_t.device)
        check(lib.dsr_pw_incr(_ptr(self.step_t), _ptr(found), st))
        # one argument block for every Adam launch of this step (dsr_adam_args: the C side reads it during each call)
        self._args = _lib.AdamArgs(_ptr(self.step_t), 0.0 if hyper else self.lr, self.betas[0], self.betas[1], self.eps,
                                   self.grad_scale, _ptr(self._hyper) if hyper else None, _ptr(scale), _ptr(found))
        args = C.byref(self._args)
        deferred, grads, factors = [], [], []     # device hyper block: the Adam launches follow the norm pass

        def launch(fn, p, sh):
            def run():
                check(fn())
                bump(p)
                if sh is not None:           # after bump(): the shadow written by this launch IS the new version
                    mark_shadow_current(p)
            if hyper:
                deferred.append(run)
            else:
                run()

        small, keep = [], []
        for p, m, v in zip(self.params, self.m, self.v):
            pending = getattr(p, "_dsr_grad_factors", None)
            if pending:
                p._dsr_grad_factors = []
                if len(pending) == 1 and p.grad is None and p.is_contiguous():
                    f = pending[0]
                    f.wait()
                    sh = shadow_for_update(p)
                    if hyper:
                        factors.append(f)
                    launch(lambda f=f, p=p, m=m, v=v, sh=sh: lib.dsr_linear_wgrad_adam(
                        f.dt, _ptr(f.dyt), _ptr(f.xt), f.bp, f.o, f.k, f.ranks, f.scale, _ptr(p), _ptr(m), _ptr(v),
                        _ptr(sh), args, st), p, sh)
                    continue
                # several backward passes since zero_grad (or a .grad from elsewhere): accumulate like autograd would
                for f in pending:
                    g = f.materialize()
                    p.grad = g if p.grad is None else p.grad + g
            if p.grad is None:
                continue
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
                keep.append(g)
            sh = shadow_for_update(p)        # bf16 image kept by DenseHead for this matrix (or None)
            # the per-tensor launch moves 16-byte vectors (dsr_pw_adam refuses anything else): a parameter that is a view
            # off such a boundary takes the multi-tensor launch, whose accesses are scalar, whatever its size
            skew = p.data_ptr() % 16 != 0 and p.numel() > 0
            if skew and (sh is not None or not p.is_contiguous()):
                idx = next(i for i, q in enumerate(self.params) if q is p)
                raise ValueError(f"FusedAdam: parameter {idx} of shape {tuple(p.shape)} starts "
                                 f"{p.data_ptr() % 16} bytes off a 16-byte boundary and "
                                 + ("has a bf16 shadow" if sh is not None else "is not contiguous")
                                 + ": the per-tensor Adam launch that would serve it needs 16-byte aligned tensors")
            multi = sh is None and p.is_contiguous() and (skew or p.numel() <= self.MULTI_MAX)
            if not multi and g.data_ptr() % 16 != 0:
                g = g.clone()                # a gradient view bound for the per-tensor launch: copied, like a strided one
                keep.append(g)
            grads.append(g)
            if multi:
                if p.numel():                # (a zero-element parameter has nothing to update, in any mode)
                    small.append((p, g, m, v))
                bump(p)                      # (rewritten by the multi-tensor launch below, before anything reads it)
                continue
            launch(lambda p=p, g=g, m=m, v=v, sh=sh: lib.dsr_pw_adam(
                _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sh), args, st), p, sh)
        if hyper:
            self._write_hyper(grads, factors, scale)
            for run in deferred:
                run()
        if small:                            # every small tensor in one launch per 64 (dsr_pw_adam_multi)
            arr = [ptr_table([t[i] for t in small]) for i in range(4)]
            ns = size_table([t[0].numel() for t in small])
            check(lib.dsr_pw_adam_multi(len(small), arr[0], arr[1], arr[2], arr[3], ns, args, st))
        # packed 16-bit conv weight images follow in one launch, not one per layer (after a skipped step the same bits again:
        # the launch sequence stays fixed for graph replay)
        repack_cached(self.params)


def _pow2_exponent(x):
    """k with x == 2**k, or None."""
    x = float(x)
    if not (x > 0 and math.isfinite(x)):
        return None
    m, e = math.frexp(x)
    return e - 1 if m == 0.5 else None


class DynamicLossScaler:
    """torch.amp.GradScaler for the 16-bit HIP training paths (the fp16 DIP net above all), with nothing read on the host:
    scale, growth counter and overflow flag are three device words, the skipped step is decided inside the kernels, so a
    whole step stays capturable in a HIP graph (steps.GraphedStep).  Constructor names, defaults and ``state_dict()`` keys
    are GradScaler's; a checkpoint moves between the two.

        scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()

    ``step`` = one pass over the gradients that raises the flag if any element is Inf / NaN (dsr_amp_check), then
    ``optimizer.step(scaler=self)``: gradients times 1 / scale, or nothing at all when the flag is up.  ``update`` applies
    torch's rule (overflow: scale *= backoff_factor; ``growth_interval`` clean steps in a row: scale *= growth_factor) and
    clears the flag.  All three factors must be powers of two: un-scaling is then exact, a run under the scaler is bit for bit
    the run under the static scale it sits at.  The state is created on the device of the first loss.

    Under data parallelism the check runs inside step(), after the gradient all-reduce, so every rank sees the same flag.
    FusedLBFGS is not served: its closure values and curvature pairs do not survive skipped steps.  ``get_scale()`` and
    ``counts()`` are the only host reads."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        kg, kb = _pow2_exponent(growth_factor), _pow2_exponent(backoff_factor)
        if _pow2_exponent(init_scale) is None:
            raise ValueError(f"init_scale must be a power of two, got {init_scale!r}")
        if kg is None or kg < 1:
            raise ValueError(f"growth_factor must be 2**k with k >= 1, got {growth_factor!r}")
        if kb is None or kb > -1:
            raise ValueError(f"backoff_factor must be 2**-k with k >= 1, got {backoff_factor!r}")
        if isinstance(growth_interval, bool) or int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError(f"growth_interval must be a positive integer, got {growth_interval!r}")
        self.enabled = bool(enabled)
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor = float(growth_factor), float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale = self._growth_tracker = self._found_inf = self._stats = None
        self._checked = False        # host side: step() has raised or left the overflow flag and update() has not cleared it yet

    def _state(self, device):
        """(scale, found_inf) device tensors, created on first use."""
        if self._scale is None:
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((1,), self._init_growth_tracker, dtype=torch.int32, device=device)
            self._found_inf = torch.zeros(1, dtype=torch.float32, device=device)
            self._stats = torch.zeros(2, dtype=torch.int32, device=device)
        return self._scale, self._found_inf

    def scale(self, loss):
        """loss * scale as a differentiable device scalar (functional.ScaleLossDevice)."""
        if not self.enabled:
            return loss
        from .functional import ScaleLossDevice
        return ScaleLossDevice.apply(loss, self._state(loss.device)[0])

    def ambient(self, device):
        """Context for callers whose loss never reaches scale(): the scale enters at the network output's backward."""
        from .functional import ambient_loss_scale
        return ambient_loss_scale(self._state(device)[0] if self.enabled else None)

    def step(self, optimizer):
        if not self.enabled:
            return optimizer.step()
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("DynamicLossScaler.step drives optim.FusedAdam (FusedLBFGS and torch optimizers are not served)")
        grads, keep = [], []
        for p in optimizer.params:
            g = p.grad
            if g is not None and g.numel() and (g.dtype != torch.float32 or not g.is_contiguous()):
                g = p.grad = g.float().contiguous()      # what FusedAdam.step would make of it; checked and applied alike
            grads.append(g if g is not None and g.numel() else None)
        _, found = self._state(optimizer.step_t.device)
        k = len(grads)
        check(_lib.lib().dsr_amp_check(k, ptr_table(grads), size_table([0 if g is None else g.numel() for g in grads]),
                                       _ptr(found), _stream()))
        self._checked = True
        return optimizer.step(scaler=self)

    def update(self):
        if not self.enabled:
            return
        if self._scale is None:
            raise RuntimeError("DynamicLossScaler.update() before any scale() or step()")
        check(_lib.lib().dsr_amp_update(_ptr(self._scale), _ptr(self._growth_tracker), _ptr(self._found_inf),
                                        self._growth_factor, self._backoff_factor, self._growth_interval,
                                        _ptr(self._stats), _stream()))
        self._checked = False

    def get_scale(self):
        """The current scale as a host float (synchronises)."""
        if not self.enabled:
            return 1.0
        return self._init_scale if self._scale is None else float(self._scale.item())

    def counts(self):
        """(steps taken, steps skipped) over all update() calls so far (one host read)."""
        if self._stats is None:
            return (0, 0)
        t, s = self._stats.tolist()
        return (t, s)

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys and meaning (empty when disabled, as there)."""
        if not self.enabled:
            return {}
        tracker = self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        if not self.enabled:
            return
        if not state_dict:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled scaler.")
        probe = DynamicLossScaler(state_dict["scale"], state_dict["growth_factor"], state_dict["backoff_factor"],
                                  state_dict["growth_interval"])      # the same argument checks
        self._init_scale, self._init_growth_tracker = probe._init_scale, int(state_dict["_growth_tracker"])
        self._growth_factor, self._backoff_factor = probe._growth_factor, probe._backoff_factor
        self._growth_interval = probe._growth_interval
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


class WeightEMA:
    """Exponential moving average of a module's weights on the device -- the copy of a GAN generator that gets evaluated and
    shipped (ESRGAN, Real-ESRGAN, SwinIR, BasicSR: ``ema_decay = 0.999``) -- as csrc/ema.hip runs it: one launch per 64 tensors
    plus a one-thread counter launch, whatever the number of averaged steps.

        ema = WeightEMA(gen, decay=0.999)
        ... opt.step(); ema.update()                                    # or: scaler.step(opt); ema.update(scaler); scaler.update()
        with ema.average_parameters(): evaluate(gen)                    # the averaged weights swapped in, and out again
        torch.save(ema.module_state_dict(), path)                       # loads into a fresh module of the same class

    ``warmup=False`` is ``AveragedModel(module, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=use_buffers)``: the
    first update copies the weights, later ones move the average by ``1 - decay`` of the difference.  ``warmup=True`` is the
    rule of timm and torch-ema: update number k (from 1) uses ``min(decay, (1 + k) / (10 + k))``, and there is no copy step:
    the average starts as the copy of the weights taken here, at construction.

    ``use_buffers=False``: every buffer is copied from the module at each update, as torch does (BatchNorm's running statistics
    are moving averages already).  ``use_buffers=True``: floating-point buffers are averaged like parameters; integer buffers
    (``num_batches_tracked``) are COPIED -- a deliberate departure from torch, which truncates ``b_ema * decay + b * (1 -
    decay)`` to an integer and so leaves such a counter behind the model's for good.

    The count of averaged steps is ``n_averaged``, an int32 device tensor [1]; which of copy and lerp an update performs is
    decided inside the kernel, so ``update()`` reads nothing on the host, issues the same launches on every call and is
    captured by steps.GraphedStep with the rest of a step (warm-up and capture calls count as updates, as they do for Adam).

    Skipped steps: ``update(scaler)`` with the optim.DynamicLossScaler that drove the optimizer reads the scaler's overflow
    word on the device; after a step the scaler skipped nothing moves, ``n_averaged`` included.  (torch's AveragedModel beside a
    GradScaler knows nothing of the skip and averages the unchanged weights once more.)  The word is cleared by
    ``scaler.update()``, so the order is ``scaler.step(opt); ema.update(scaler); scaler.update()``; anything else raises.

    ``swap()`` / ``copy_to()`` / ``restore()`` rewrite live tensors through their raw pointers and then do what FusedAdam does
    after its own launches: every rewritten tensor's version is advanced (functional.bump), so the packed 16-bit conv weight
    images are re-packed here (functional.repack_cached), an eval-mode BatchNorm's kept affine map is formed again, and the bf16
    shadow of a dense-head matrix is cast again at its next use.

    Parameters must be contiguous fp32 (what FusedAdam trains); buffers contiguous with a byte size that is a multiple of four."""

    def __init__(self, module, decay=0.999, warmup=False, use_buffers=False):
        self.module = module
        self.decay, self.warmup, self.use_buffers = self._checked_decay(decay), bool(warmup), bool(use_buffers)
        self._slots = []             # (name, owner, key, is_buffer): the live tensor is looked up at every call (.to() replaces buffers)
        seen = set()
        for is_buffer, table in ((False, "_parameters"), (True, "_buffers")):
            for prefix, owner in module.named_modules():
                for key, t in getattr(owner, table).items():
                    if t is None or id(t) in seen:
                        continue
                    seen.add(id(t))
                    self._slots.append(((prefix + "." if prefix else "") + key, owner, key, is_buffer))
        if not any(not s[3] for s in self._slots):
            raise ValueError("WeightEMA got a module without parameters")
        live = self._live()
        for (name, _, _, is_buffer), t in zip(self._slots, live):
            if not is_buffer and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise TypeError(f"WeightEMA takes contiguous fp32 parameters; {name} is {t.dtype}, contiguous={t.is_contiguous()}")
            if is_buffer and (not t.is_contiguous() or t.numel() * t.element_size() % 4):
                raise TypeError(f"WeightEMA takes contiguous buffers of a multiple of 4 bytes; {name} is {t.dtype} "
                                f"{tuple(t.shape)}, contiguous={t.is_contiguous()}")
            if is_buffer and self.use_buffers and t.is_floating_point() and t.dtype != torch.float32:
                raise TypeError(f"WeightEMA(use_buffers=True) averages fp32 buffers; {name} is {t.dtype}")
        self._shadow = [t.detach().clone(memory_format=torch.contiguous_format) for t in live]
        self.n_averaged = torch.zeros(1, dtype=torch.int32, device=live[0].device)
        self._backup = None

    @staticmethod
    def _checked_decay(decay):
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:     # (NaN fails too)
            raise ValueError(f"Invalid decay value {decay!r} provided. Please provide a value in [0,1] range.")   # torch's words
        return float(decay)

    # ------------------------------------------------------------------ tables
    def _live(self):
        return [getattr(owner, "_buffers" if is_buffer else "_parameters")[key] for _, owner, key, is_buffer in self._slots]

    def _copied(self, i):
        """Is slot i copied from the module (not averaged)?"""
        return self._slots[i][3] and not (self.use_buffers and self._shadow[i].is_floating_point())

    def _on_device(self, live):
        """The tensors of an operation that runs on the HIP path: on the GPU, the state beside them."""
        _need_gpu(live[0])
        dev = live[0].device
        for (name, _, _, _), t, sh in zip(self._slots, live, self._shadow):
            if t.device != dev or t.shape != sh.shape or t.dtype != sh.dtype or not t.is_contiguous():
                raise RuntimeError(f"WeightEMA: {name} is now {t.dtype} {tuple(t.shape)} on {t.device}, contiguous="
                                   f"{t.is_contiguous()}; the average holds {sh.dtype} {tuple(sh.shape)} for {dev}")
        if self.n_averaged.device != dev:          # the module was moved after construction: the state follows it
            self._shadow = [sh.to(dev) for sh in self._shadow]
            self.n_averaged = self.n_averaged.to(dev)
            if self._backup is not None:
                self._backup = [b.to(dev) for b in self._backup]

    @staticmethod
    def _tables(dst, src):
        """HOST tables of the C ABI over 32-bit words (a copy or a swap moves bits, so an int64 counter is two words each)."""
        k = len(dst)
        return k, ptr_table(dst), ptr_table(src), size_table([t.numel() * t.element_size() // 4 for t in dst])

    def _rewritten(self, module, tensors):
        for t in tensors:
            bump(t)
        repack_cached(list(module.parameters()))

    def _copy_exact(self, dst, src):
        """dst[i] <- src[i], bit for bit (the update launch with every tensor flagged `copy`)."""
        k, d, s_, n = self._tables(dst, src)
        check(_lib.lib().dsr_ema_update_multi(k, d, s_, n, (C.c_ubyte * k)(*([1] * k)), 0.0, 0, _ptr(self.n_averaged), None,
                                              _stream()))

    # ------------------------------------------------------------------ the step
    def update(self, scaler=None):
        """One averaging step, after ``opt.step()``.  ``scaler``: the optim.DynamicLossScaler whose ``step(opt)`` has just run
        and whose ``update()`` has not (see the class docstring)."""
        live = self._live()
        self._on_device(live)
        found = None
        if scaler is not None and scaler.enabled:
            if not scaler._checked:
                raise RuntimeError("WeightEMA.update(scaler): the scaler's overflow flag of this step is gone -- the order is "
                                   "scaler.step(opt); ema.update(scaler); scaler.update()")
            found = scaler._state(live[0].device)[1]
        lib, st = _lib.lib(), _stream()
        k, sh, p, n = self._tables(self._shadow, live)
        flags = (C.c_ubyte * k)(*[1 if self._copied(i) else 0 for i in range(k)])
        check(lib.dsr_ema_update_multi(k, sh, p, n, flags, self.decay, 1 if self.warmup else 0, _ptr(self.n_averaged),
                                       _ptr(found), st))
        check(lib.dsr_ema_tick(_ptr(self.n_averaged), _ptr(found), st))

    # ------------------------------------------------------------------ the averaged weights in a live module
    def swap(self):
        """Exchange the module's tensors with the average, bit for bit; a second call undoes the first."""
        live = self._live()
        self._on_device(live)
        k, a, b, n = self._tables(live, self._shadow)
        check(_lib.lib().dsr_ema_swap_multi(k, a, b, n, _stream()))
        self._rewritten(self.module, live)

    @contextlib.contextmanager
    def average_parameters(self):
        """``with ema.average_parameters():`` -- the module holds the averaged weights (and the average's buffers) inside the
        block and its own again afterwards, also when the block raises."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def copy_to(self, module=None):
        """Write the average into ``module`` (same tensor names, shapes and dtypes, on the GPU).  Default: the EMA's own module,
        whose tensors are kept aside first so that ``restore()`` can bring them back."""
        own = module is None or module is self.module
        if own:
            live = self._live()
            self._on_device(live)
            self._backup = [t.detach().clone() for t in live]
            self._copy_exact(live, self._shadow)
            self._rewritten(self.module, live)
            return
        theirs = dict(module.named_parameters())
        theirs.update(dict(module.named_buffers()))
        dst = []
        for (name, _, _, _), sh in zip(self._slots, self._shadow):
            t = theirs.get(name)
            if t is None or t.shape != sh.shape or t.dtype != sh.dtype or not t.is_contiguous():
                raise RuntimeError(f"WeightEMA.copy_to: the target has no contiguous {sh.dtype} {tuple(sh.shape)} tensor {name}")
            _need_gpu(t)
            dst.append(t)
        self._on_device(self._live())
        self._copy_exact(dst, self._shadow)
        self._rewritten(module, dst)

    def restore(self):
        """Undo one ``copy_to()`` onto the EMA's own module."""
        if self._backup is None:
            raise RuntimeError("WeightEMA.restore() without a copy_to() onto the EMA's own module before it")
        live = self._live()
        self._on_device(live)
        self._copy_exact(live, self._backup)
        self._backup = None
        self._rewritten(self.module, live)

    # ------------------------------------------------------------------ checkpoints
    def module_state_dict(self):
        """The averaged weights under the module's own ``state_dict()`` keys, order and dtypes (copies): what
        ``module.load_state_dict`` and evaluate.save_model's file format take."""
        mine = {id(t): sh for t, sh in zip(self._live(), self._shadow)}
        out = OrderedDict()
        for key, t in self.module.state_dict(keep_vars=True).items():
            sh = mine.get(id(t))
            out[key] = (t if sh is None else sh).detach().clone()
        return out

    def state_dict(self):
        """``shadow`` (name -> tensor, parameters then buffers), ``n_averaged`` (host int: one read), ``decay``, ``warmup``,
        ``use_buffers``."""
        return {"shadow": OrderedDict((s[0], sh.detach().clone()) for s, sh in zip(self._slots, self._shadow)),
                "n_averaged": int(self.n_averaged.item()), "decay": self.decay, "warmup": self.warmup,
                "use_buffers": self.use_buffers}

    def load_state_dict(self, state_dict):
        shadow = state_dict["shadow"]
        names = [s[0] for s in self._slots]
        if list(shadow.keys()) != names:
            odd = sorted(set(shadow.keys()) ^ set(names))
            raise RuntimeError(f"WeightEMA.load_state_dict: tensor names differ from the module's: {odd or 'order'}")
        decay = self._checked_decay(state_dict["decay"])
        for name, sh in zip(names, self._shadow):
            src = shadow[name]
            if src.shape != sh.shape or src.dtype != sh.dtype:
                raise RuntimeError(f"WeightEMA.load_state_dict: {name} is {src.dtype} {tuple(src.shape)}, expected "
                                   f"{sh.dtype} {tuple(sh.shape)}")
        with torch.no_grad():
            for name, sh in zip(names, self._shadow):
                sh.copy_(shadow[name])
            self.n_averaged.fill_(int(state_dict["n_averaged"]))
        self.decay, self.warmup, self.use_buffers = decay, bool(state_dict["warmup"]), bool(state_dict["use_buffers"])


class FusedLBFGS:
    """torch.optim.LBFGS (line_search_fn=None) with the same constructor, defaults, closure calls and stopping rules,
    run by csrc/lbfgs.hip: per closure call one gather pass over the gradients, one dot pass and one combine pass over
    the history, and a one-wave fp64 kernel that runs the two-loop recursion on the Gram matrix of {s_i, y_i, g} and
    decides every break of torch's loop.  The whole state (history ring, Gram matrix, n_iter, func_evals, d, t, H_diag,
    prev_loss) lives on the device and persists across step() calls; the only host read is the 4-byte stop flag after
    each closure call.  Parameters: contiguous fp32 dense tensors on the device."""
    MAX_HISTORY = 1024       # the scalar kernel keeps its coefficient vectors in LDS

    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                 history_size=100, line_search_fn=None):
        if line_search_fn is not None:
            if line_search_fn == "strong_wolfe":
                raise NotImplementedError("FusedLBFGS: line_search_fn='strong_wolfe' is not implemented; only the fixed "
                                          "step (line_search_fn=None) runs on the HIP path")
            raise ValueError("only 'strong_wolfe' is supported")      # torch.optim.LBFGS's own message
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 1 <= int(history_size) <= self.MAX_HISTORY:
            raise ValueError(f"history_size must be in [1, {self.MAX_HISTORY}], got {history_size}")
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        for i, p in enumerate(self.params):
            if (not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.layout != torch.strided
                    or not p.is_contiguous() or not p.is_cuda):
                what = type(p).__name__ if not isinstance(p, torch.Tensor) else \
                    f"{p.dtype}, {p.layout}, contiguous={p.is_contiguous()}, device={p.device}"
                raise TypeError(f"FusedLBFGS takes contiguous fp32 dense parameters on the device; parameter {i} is {what}")
        self.lr, self.max_iter = float(lr), int(max_iter)
        self.max_eval = int(max_iter * 5 // 4 if max_eval is None else max_eval)
        self.tolerance_grad, self.tolerance_change = float(tolerance_grad), float(tolerance_change)
        self.history_size = int(history_size)
        self._flat = [p for p in self.params if p.numel() > 0]      # what the flat vector is made of (torch's order)
        self.n = sum(p.numel() for p in self._flat)
        k = len(self._flat)
        lib = _lib.lib()
        self._ws_bytes = lib.dsr_lbfgs_workspace(self.history_size, self.n, k) if k else 0
        nvec = lib.dsr_lbfgs_vector_floats(self.history_size, self.n) if k else 0
        if not self._ws_bytes or not nvec:
            raise ValueError(f"FusedLBFGS: no state for history_size={history_size} over {self.n} elements")
        dev = self.params[0].device
        self._ws = torch.zeros(self._ws_bytes, dtype=torch.uint8, device=dev)
        self._vecs = torch.zeros(nvec, dtype=torch.float32, device=dev)
        self._stop = torch.zeros(1, dtype=torch.int32, device=dev)
        self._numel = size_table([p.numel() for p in self._flat])

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def state_counts(self):
        """Host ints of the device counters (one read; for tests): state["n_iter"], state["func_evals"] of torch's
        optimizer, the iterations and closure calls of the last step(), and the pairs held in the history."""
        v = self._ws[:20].cpu().view(torch.int32).tolist()
        return {"n_iter": v[0], "func_evals": v[1], "step_iters": v[2], "step_evals": v[3], "history": v[4]}

    def _loss_scalar(self, loss):
        if isinstance(loss, torch.Tensor):
            return loss.detach().to(device=self._ws.device, dtype=torch.float32).reshape(1).contiguous()
        return torch.full((1,), float(loss), dtype=torch.float32, device=self._ws.device)

    def _pass(self, loss, first):
        """gather, dots, scalar, combine for one closure value; the parameters move (or not) on the device."""
        lib = _lib.lib()
        st = _stream()
        k, h, n = len(self._flat), self.history_size, self.n
        grads = []
        for p in self._flat:
            g = p.grad
            if g is not None and g.is_sparse:
                g = g.to_dense()
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous()):
                g = g.float().contiguous()
            grads.append(g)
        lv = self._loss_scalar(loss)
        ws, vecs = _ptr(self._ws), _ptr(self._vecs)
        check(lib.dsr_lbfgs_gather(k, ptr_table(grads), self._numel, ws, self._ws_bytes, vecs, h, n, st))
        check(lib.dsr_lbfgs_dots(ws, self._ws_bytes, vecs, h, n, k, st))
        check(lib.dsr_lbfgs_scalar(ws, self._ws_bytes, h, n, k, _ptr(lv), 1 if first else 0, _ptr(self._stop), self.lr,
                                   self.max_iter, self.max_eval, self.tolerance_grad, self.tolerance_change, st))
        check(lib.dsr_lbfgs_combine(k, ptr_table(self._flat), self._numel, ws, self._ws_bytes, vecs, h, n, st))
        for p in self._flat:
            bump(p)
        repack_cached(self.params)

    @torch.no_grad()
    def step(self, closure):
        """lbfgs.py:333-537 without a line search: returns the first closure's value; calls the closure exactly as often as
        torch.optim.LBFGS does (the decision to call it again is the device flag, read once per call)."""
        closure = torch.enable_grad()(closure)
        orig_loss = closure()
        self._pass(orig_loss, True)
        while not int(self._stop.item()):
            self._pass(closure(), False)
        return orig_loss
