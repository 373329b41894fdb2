#!/usr/bin/env python
"""Generate tests/golden/downsampler_dense.npz by IMPORTING the reference's own Downsampler (build container only).

For each case of tests/downsampler_dense_ref.CASES the reference module is built, moved to float64, its Conv2d weight and
bias get a seeded dense perturbation (so that every filter and the bias are live, as after get_params('down') training),
and x, w, b, the probe dy, y and the gradients dx, dw, db of sum(y * dy) are recorded as float32.  The file holds only
what the reference computed; the reference's Python never travels to the GPU machine.

    python tests/golden/make_golden_downsampler_dense.py"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

from downsampler_dense_ref import CASES  # noqa: E402
from utils.downsampler import Downsampler  # noqa: E402  (reference)


def main():
    out = {}
    for idx, (name, (kw, shape)) in enumerate(CASES.items()):
        rng = np.random.RandomState(1234 + idx)
        with contextlib.redirect_stdout(io.StringIO()):    # the gauss branch prints
            d = Downsampler(**kw).double()
        w0 = d.downsampler_.weight.detach().numpy()
        w = w0 + rng.standard_normal(w0.shape) * np.abs(w0).max() * 0.25
        b = rng.standard_normal(w0.shape[0]) * 0.1
        # what travels is float32: the float64 module computes on exactly those values
        w, b = w.astype(np.float32), b.astype(np.float32)
        x = rng.uniform(0.0, 1.0, shape).astype(np.float32)
        with torch.no_grad():
            d.downsampler_.weight.copy_(torch.from_numpy(w).double())
            d.downsampler_.bias.copy_(torch.from_numpy(b).double())
        xt = torch.from_numpy(x).double().requires_grad_(True)
        y = d(xt)
        dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
        (y * torch.from_numpy(dy).double()).sum().backward()
        for key, val in (("x", x), ("w", w), ("b", b), ("dy", dy), ("y", y.detach().numpy()), ("dx", xt.grad.numpy()),
                         ("dw", d.downsampler_.weight.grad.numpy()), ("db", d.downsampler_.bias.grad.numpy())):
            out[f"{name}.{key}"] = np.asarray(val, dtype=np.float32)
    path = os.path.join(HERE, "downsampler_dense.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
