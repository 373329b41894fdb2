"""Float64 CPU yardstick of the spectral-norm kernels (csrc/spectral_norm.hip): the power iteration, the eval-mode sigma and
the backward of torch.nn.utils.spectral_norm(conv) with n_power_iterations = 1, restated with plain matrix products.
tests/test_host_unetd.py holds these formulas to torch's own hook.  Nothing is imported from the package under test."""
import torch

EPS = 1e-12


def mat(w):
    return w.double().reshape(w.shape[0], -1)


def iterate(w, u, v, eps=EPS):
    """One train-mode forward: (u', v', sigma, W_sn) from the weight (any shape with Cout first) and the stored vectors."""
    W = mat(w)
    t = W.t() @ u.double()
    v = t / max(float(t.norm()), eps)
    s = W @ v
    u = s / max(float(s.norm()), eps)
    sigma = u @ s
    return u, v, sigma, w.double() / sigma


def evaluate(w, u, v):
    """Eval mode: (sigma, W_sn) from the stored vectors, which stay as they are."""
    sigma = u.double() @ (mat(w) @ v.double())
    return sigma, w.double() / sigma


def backward(g, w_sn, u, v, sigma):
    """dL/dW from G = dL/dW_sn with u, v (of that forward) as constants: (G - <G, W_sn> u v^T) / sigma."""
    G = mat(g)
    d = (G * mat(w_sn)).sum()
    return ((G - d * torch.outer(u.double(), v.double())) / sigma).reshape(g.shape)


def hadamard(n):
    """Sylvester's n x n Hadamard matrix (n a power of two), entries +-1, float64."""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h
