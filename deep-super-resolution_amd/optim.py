"""Adam with torch.optim.Adam's default semantics (train_GAN.py:35-36, utils/DIP.py:34) as one fused
HIP kernel per tensor; the step counter lives on the device so a whole train step can be captured
in a HIP graph.  L-BFGS with torch.optim.LBFGS's semantics (utils/DIP.py:24-31) as four HIP passes
per closure call, its whole state on the device."""
import ctypes as C

import torch

from . import _lib
from .functional import _ptr, _stream, bump, check, mark_shadow_current, repack_cached, shadow_for_update


class FusedAdam:
    MULTI_MAX = 1 << 20      # tensors up to this many elements go through the multi-tensor launch

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, fuse_dense_head=False):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")   # torch.optim raises the same
        # fuse_dense_head: the dense head's big matrix (discriminator.py:54, marked `_dsr_dense_head`) gets its gradient as
        # two 16-bit factors (functional.GradFactors) instead of a `.grad` tensor, and step() applies Adam inside the
        # weight-gradient contraction (dsr_linear_wgrad_adam).  Same arithmetic, bit for bit; `.grad` of that one tensor
        # stays None, which is why it is opt-in (steps / bench turn it on, nothing else reads that gradient).
        self.fuse_dense_head = bool(fuse_dense_head)
        if self.fuse_dense_head:
            for p in self.params:
                if getattr(p, "_dsr_dense_head", False):
                    p._dsr_defer_wgrad = True
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        self.grad_scale = float(grad_scale)     # gradients are multiplied by this first (1/S for a loss scale S)
        dev = self.params[0].device
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if getattr(p, "_dsr_grad_factors", None):
                p._dsr_grad_factors = []
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def step(self):
        lib = _lib.lib()
        st = _stream()
        check(lib.dsr_pw_incr(_ptr(self.step_t), st))
        small, keep = [], []
        for p, m, v in zip(self.params, self.m, self.v):
            pending = getattr(p, "_dsr_grad_factors", None)
            if pending:
                p._dsr_grad_factors = []
                if len(pending) == 1 and p.grad is None and p.is_contiguous():
                    f = pending[0]
                    f.wait()
                    sh = shadow_for_update(p)
                    check(lib.dsr_linear_wgrad_adam(f.dt, _ptr(f.dyt), _ptr(f.xt), f.bp, f.o, f.k, f.ranks, f.scale, _ptr(p),
                                                    _ptr(m), _ptr(v), _ptr(sh), _ptr(self.step_t), self.lr, self.betas[0],
                                                    self.betas[1], self.eps, self.grad_scale, st))
                    bump(p)
                    if sh is not None:
                        mark_shadow_current(p)
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
            if sh is None and p.numel() <= self.MULTI_MAX and p.is_contiguous():
                small.append((p, g, m, v))
            else:
                check(lib.dsr_pw_adam(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), self.lr, self.betas[0],
                                      self.betas[1], self.eps, _ptr(self.step_t), self.grad_scale, _ptr(sh), st))
            bump(p)
            if sh is not None:               # after bump(): the shadow written by this launch IS the new version
                mark_shadow_current(p)
        if small:                            # every small tensor in one launch per 64 (dsr_pw_adam_multi)
            k = len(small)
            arr = [(C.c_void_p * k)(*[t[i].data_ptr() for t in small]) for i in range(4)]
            ns = (C.c_size_t * k)(*[t[0].numel() for t in small])
            check(lib.dsr_pw_adam_multi(k, arr[0], arr[1], arr[2], arr[3], ns, self.lr, self.betas[0], self.betas[1],
                                        self.eps, _ptr(self.step_t), self.grad_scale, st))
        repack_cached(self.params)           # packed 16-bit conv weight images follow in one launch, not one per layer


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
        self._numel = (C.c_size_t * k)(*[p.numel() for p in self._flat])

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
        keep, grads = [], []
        for p in self._flat:
            g = p.grad
            if g is None:
                grads.append(None)
                continue
            if g.is_sparse:
                g = g.to_dense()
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            keep.append(g)
            grads.append(g.data_ptr())
        lv = self._loss_scalar(loss)
        ws, vecs = _ptr(self._ws), _ptr(self._vecs)
        check(lib.dsr_lbfgs_gather(k, (C.c_void_p * k)(*grads), self._numel, ws, self._ws_bytes, vecs, h, n, st))
        check(lib.dsr_lbfgs_dots(ws, self._ws_bytes, vecs, h, n, k, st))
        check(lib.dsr_lbfgs_scalar(ws, self._ws_bytes, h, n, k, _ptr(lv), 1 if first else 0, _ptr(self._stop), self.lr,
                                   self.max_iter, self.max_eval, self.tolerance_grad, self.tolerance_change, st))
        check(lib.dsr_lbfgs_combine(k, (C.c_void_p * k)(*[p.data_ptr() for p in self._flat]), self._numel, ws,
                                    self._ws_bytes, vecs, h, n, st))
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
