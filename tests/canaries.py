"""Sentinel-filled output buffers for the tests that call the raw C ABI (test_gpu_pointwise.py, test_gpu_resample.py).

A kernel that stores outside its output cannot be seen in the output itself.  Every output of such a call is therefore a view
into a larger buffer filled with SENTINEL; check() asserts that the MARGIN elements on each side of every view still hold it.
MARGIN is a multiple of 8 elements, so a view of 16-bit data starts on a 16-byte boundary like the tensors of the product."""
import torch

SENTINEL = 7777.0
MARGIN = 512          # elements on each side of an output


class Canaries:
    """Outputs allocated inside sentinel-filled buffers; check() asserts that nothing outside an output was written."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def alloc(self, shape, dtype, what):
        numel = 1
        for s in shape:
            numel *= int(s)
        flat = torch.full((numel + 2 * MARGIN,), SENTINEL, dtype=dtype, device=self.dev)
        self.bufs.append((flat, numel, what))
        return flat[MARGIN:MARGIN + numel].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for flat, numel, what in self.bufs:
            lo, hi = flat[:MARGIN], flat[MARGIN + numel:]
            assert bool((lo == lo[0]).all()) and bool((hi == lo[0]).all()) and bool(lo[0] == flat.new_tensor(SENTINEL)), \
                f"store outside {what}"

    def untouched(self, view):
        return bool((view == view.new_tensor(SENTINEL)).all())
