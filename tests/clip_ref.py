"""float64 numpy model of optim.FusedAdam(max_grad_norm=c): torch.nn.utils.clip_grad_norm_(params, c, norm_type=2.0,
error_if_nonfinite=False) followed by torch.optim.Adam (defaults: no weight decay, no amsgrad).

The gradients handed to step() are the RAW ones (what backward left, still multiplied by a loss scale if there is one);
``grad_scale`` takes the scale out first, as the kernels do, so the norm is that of the true gradient.  Only the arithmetic
differs from the device: plain float64 numpy here, fp32 kernels with fp64 partial sums there."""
import numpy as np


def total_norm(grads, grad_scale=1.0):
    """2-norm over every gradient that is not None, of the gradients times grad_scale."""
    s = 0.0
    for g in grads:
        if g is not None:
            g = np.asarray(g, dtype=np.float64)
            s += float((g * g).sum())
    return np.sqrt(s) * abs(grad_scale)


def clip_coef(norm, max_norm):
    """torch's coefficient: min(1, max_norm / (norm + 1e-6)); NaN stays NaN."""
    c = max_norm / (norm + 1e-6)
    return c if c != c else min(c, 1.0)


class ClippedAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_grad_norm=None):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        self.grad_scale, self.max_grad_norm = float(grad_scale), max_grad_norm
        self.t = 0
        self.grad_norm = self.clip_coef = None

    def step(self, grads, lr=None):
        """One update; a parameter whose gradient is None is left alone (and out of the norm).  `lr`: this step's rate."""
        lr = self.lr if lr is None else float(lr)
        self.grad_norm = total_norm(grads, self.grad_scale)
        self.clip_coef = 1.0 if self.max_grad_norm is None else clip_coef(self.grad_norm, self.max_grad_norm)
        mult = self.grad_scale * self.clip_coef
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64) * mult
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            self.p[i] = self.p[i] - (lr / bc1) * (self.m[i] / (np.sqrt(self.v[i]) / np.sqrt(bc2) + self.eps))
