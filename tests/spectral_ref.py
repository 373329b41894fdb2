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


# ----------------------------------------------------------------------------- the launch group's partition, restated
MAX_LAYERS = 64              # layers of one call (csrc/multi_tensor.h, DSR_MT_MAX)
V_THREADS = 1024             # sn_v_kernel: one block per layer; a thread takes 4 columns a turn on the 16-byte path, else 1
ROWS, CHUNK = 32, 4096       # rows of W behind one W^T u partial; elements of W per block of the streaming kernels

WIDE_VECTOR = (256, 4608)    # UNetDiscriminatorSN(num_feat=64).conv4: K > 4096, a second turn on the 16-byte path
WIDE_SCALAR = (32, 1152)     # K > 1024: a second turn on the 4-byte path (reached with pointers off their 16-byte boundary)
# 64 layers of one call: small mixed shapes, K % 4 != 0 ((8, 27), (7, 33), (12, 37)) and Cout % 32 != 0 (all but (32, 256) and (64, 64))
FULL_TABLE = [(8, 27), (16, 128), (130, 52), (7, 33), (32, 256), (12, 37), (64, 64), (24, 100)] * 8


def v_turns(k, vec):
    """Turns of sn_v_kernel's column loops for a layer of K columns."""
    return -(-k // (V_THREADS * (4 if vec else 1)))


def _r4(x):
    return (x + 3) & ~3


def fwd_workspace_bytes(shapes):
    """dsr_spectral_norm_workspace: per layer s [round_up(Cout, 4)], then ceil(Cout / 32) partial rows of K floats, rounded up to 4."""
    return 4 * sum(_r4(c) + _r4(-(-c // ROWS) * k) for c, k in shapes)


def bwd_workspace_bytes(shapes):
    """dsr_spectral_norm_bwd_workspace: per layer one partial per 4096 elements, rounded up to 4."""
    return 4 * sum(_r4(-(-(c * k) // CHUNK)) for c, k in shapes)


def hadamard(n):
    """Sylvester's n x n Hadamard matrix (n a power of two), entries +-1, float64."""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h
