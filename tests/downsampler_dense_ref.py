"""Restatement of the reference Downsampler as the dense layer it is (test infrastructure, differentiable): ReplicationPad2d(pad)
followed by Conv2d(n_planes, n_planes, k, stride=factor) with a bias, every filter live.  Written with torch's own pad and
conv2d, so torch autograd of it is the reference gradient of the GPU tests; it runs in whatever dtype its inputs have (float64
for the reference, float32 for the floor that a different but equally long summation order is measured against).
tests/golden/downsampler_dense.npz pins it to the reference module itself."""
import torch
import torch.nn.functional as F


def downsample_dense(x, weight, bias, factor, pad):
    """y[n,co,oy,ox] = b[co] + sum_ci sum_ij w[co,ci,i,j] x[n,ci,clamp(oy f + i - pad),clamp(ox f + j - pad)]."""
    if pad:
        x = F.pad(x, (pad, pad, pad, pad), mode="replicate")
    return F.conv2d(x, weight, bias, stride=factor)


def grads(x, weight, bias, dy, factor, pad, dtype=torch.float64):
    """(y, dx, dw, db) of sum(y * dy) in `dtype` on the CPU."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    w = weight.detach().cpu().to(dtype).requires_grad_(True)
    b = bias.detach().cpu().to(dtype).requires_grad_(True)
    y = downsample_dense(x, w, b, factor, pad)
    (y * dy.detach().cpu().to(dtype)).sum().backward()
    return y.detach(), x.grad, w.grad, b.grad


def pad_of(kernel_size, factor, preserve_size):
    """The reference's padding rule (utils/downsampler.py:54-61)."""
    if not preserve_size:
        return 0
    return (kernel_size - 1) // 2 if kernel_size % 2 == 1 else (kernel_size - factor) // 2


# the golden cases: name -> (constructor kwargs, input shape)
CASES = {
    "l2_f2": (dict(n_planes=3, factor=2, kernel_type="lanczos2", phase=0.5, preserve_size=True), (1, 3, 40, 48)),
    "l2_f4": (dict(n_planes=3, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True), (1, 3, 40, 48)),
    "l2_f8": (dict(n_planes=3, factor=8, kernel_type="lanczos2", phase=0.5, preserve_size=True), (1, 3, 48, 64)),
    "l3_f2_nopad": (dict(n_planes=3, factor=2, kernel_type="lanczos3", phase=0, preserve_size=False), (1, 3, 36, 44)),
    "g12": (dict(n_planes=3, factor=2, kernel_type="gauss12", phase=0, preserve_size=True), (1, 3, 32, 40)),
    "planes1": (dict(n_planes=1, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True), (1, 1, 40, 48)),
    "ragged": (dict(n_planes=3, factor=4, kernel_type="lanczos2", phase=0.5, preserve_size=True), (1, 3, 37, 43)),
    "batch2": (dict(n_planes=3, factor=2, kernel_type="lanczos3", phase=0, preserve_size=True), (2, 3, 24, 28)),
}
