"""GPU: the blind-degradation kernel (csrc/degrade.hip) at every scale, through the raw C ABI, bit for bit against
tests/degrade_ref.py on the data of tests/degrade_sweep_ref.py (the exact regime, the kernel families and the wrong variants that
this data tells apart: that file and tests/test_host_degrade_sweep.py).  tests/test_gpu_degrade.py compares scales 1, 2, 3, 4 and 8
bit for bit, scale 5 to one grey level and scales 6 and 7 not at all, with point-symmetric kernels throughout; here

  every S in 1..8         all eight instantiations of degrade_kernel<S> and their LDS layouts, on an LR grid of 2 x 3 (16-row
                          tiles) or 3 x 3 (8-row tiles) ragged tiles, every odd ks in 1..21, offsets {0, S // 2, S - 1}
  unsymmetric kernels     taps walked backwards or a transposed kernel give other numbers
  a signed kernel         outputs beyond both clips
  a two-tap kernel        .5 ties under rintf
  the smallest images     (ks // 2 + 1) square: the footprint reflects off both borders at once

each as one whole-grid patch per sample of dsr_degrade_batch_u8 (two samples: the unsymmetric and the signed kernel) and as
dsr_degrade_image_u8.  Float outputs are pre-filled with NaN, byte outputs with 0xA5; all sit between sentinel margins, and the
images and kernels between margins of their own."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import degrade_sweep_ref as S

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
NAN = float("nan")
MARGIN = 1024
FAMILIES = list(S.FAMILIES)               # sample 0: unsymmetric, sample 1: signed


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    yield torch.device("cuda:0")
    S.clear()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view({1: torch.uint8, 4: torch.int32}[t.element_size()])


class Raw:
    """Device buffers between MARGIN sentinel elements on each side; check() asserts that every margin kept its bits."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, shape, dtype, fill, margin):
        numel = math.prod(shape)
        flat = torch.full((numel + 2 * MARGIN,), margin, dtype=dtype, device=self.dev)
        flat[MARGIN:MARGIN + numel] = fill
        self.bufs.append((flat, _bits(flat[:MARGIN]).clone(), _bits(flat[-MARGIN:]).clone()))
        return flat[MARGIN:MARGIN + numel].view(shape)

    def out_f32(self, shape):
        return self.new(shape, torch.float32, NAN, 7777.0)

    def out_u8(self, shape):
        return self.new(shape, torch.uint8, 0xA5, 0x5A)

    def put(self, t):
        v = self.new(tuple(t.shape), t.dtype, 0, NAN if t.dtype == torch.float32 else 0xC3)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, lo, hi in self.bufs:
            assert torch.equal(_bits(flat[:MARGIN]), lo) and torch.equal(_bits(flat[-MARGIN:]), hi), "write outside a buffer"


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _batch(raw, img, shape, kernels, ks, s, offset, quantise):
    """dsr_degrade_batch_u8 with one whole-grid patch per kernel of `kernels` (device fp32 [n, ks, ks]): fp32 [n, 3, h, w]."""
    L = P("_lib")
    n = kernels.shape[0]
    h, w = S.grid(shape, s, offset)
    out = raw.out_f32((n, 3, h, w))
    ptrs = (C.c_void_p * n)(*[img.data_ptr()] * n)
    L.check(L.lib().dsr_degrade_batch_u8(n, ptrs, _ints(*[shape[0]] * n), _ints(*[shape[1]] * n), _ints(*[0] * n), _ints(*[0] * n), None,
                                         h, w, s, offset, _ptr(kernels), ks, None, None, int(quantise), 0, _ptr(out), _st()))
    return out


def _image(raw, img, shape, kernel, ks, s, offset):
    """dsr_degrade_image_u8 under one kernel (device fp32 [ks, ks]): uint8 [h, w, 3]."""
    L = P("_lib")
    h, w = S.grid(shape, s, offset)
    out = raw.out_u8((h, w, 3))
    L.check(L.lib().dsr_degrade_image_u8(_ptr(img), shape[0], shape[1], s, offset, _ptr(kernel), ks, None, None, _ptr(out), _st()))
    return out


def _sweep(dev, which, key, host, ks, s, offs, families=FAMILIES):
    """Both entry points on one image under the kernels of size ks, every offset of `offs`, quantised and not; the outputs are
    fetched after all launches and compared with ==."""
    raw = Raw(dev)
    shape = host.shape[:2]
    img = raw.put(torch.from_numpy(host))
    make = lambda f: S.two_tap() if f == "two_tap" else S.FAMILIES[f](ks)
    kernels = raw.put(torch.from_numpy(np.stack([make(f) for f in families])))
    runs = []
    for o in offs:
        for quantise in (True, False):
            runs.append(("batch", o, quantise, _batch(raw, img, shape, kernels, ks, s, o, quantise)))
        for b in range(len(families)):
            runs.append(("image", o, b, _image(raw, img, shape, kernels[b], ks, s, o)))
    raw.check()
    assert np.array_equal(img.cpu().numpy(), host)
    for kind, o, arg, out in runs:
        got = out.cpu()
        if kind == "batch":
            assert not bool(torch.isnan(got).any()), (which, key, ks, s, o, "an output element was not written")
            for b, f in enumerate(families):
                want = S.as_f32(S.lr(S.full_blur(which, key, f, ks), s, o, arg))
                assert torch.equal(got[b], want), (kind, f, ks, s, o, arg, float((got[b] - want).abs().max()) * 255.0)
        else:
            want = S.as_u8(S.lr(S.full_blur(which, key, families[arg], ks), s, o, True))
            assert torch.equal(got, want), (kind, families[arg], ks, s, o,
                                            int((got.int() - want.int()).abs().max()), int((got != want).sum()))


@pytest.mark.parametrize("s", S.SCALES)
def test_every_kernel_size_and_offset_at_this_scale(dev, s):
    """The (20 s + 3) x (35 s + 5) image of this scale, every odd ks in 1..21, offsets {0, s // 2, s - 1}, quantised and not, as
    one two-sample batch (unsymmetric and signed kernel) and as two whole-image calls; at ks = 3 the two-tap kernel as well."""
    host = S.image(s)
    for ks in S.KS:
        _sweep(dev, "sweep", s, host, ks, s, S.offsets(s))
    _sweep(dev, "sweep", s, host, 3, s, S.offsets(s), families=["two_tap", "unsymmetric"])
    S.full_blur.cache_clear()


@pytest.mark.parametrize("s", [1, 8])
def test_smallest_legal_images(dev, s):
    """(ks // 2 + 1) square, every odd ks: at s = 1 every LR pixel reflects off both borders, at s = 8 the grid is one or two
    pixels a side."""
    for ks in S.KS:
        _sweep(dev, "small", ks, S.small_image(ks), ks, s, S.small_offsets(ks, s))
    S.full_blur.cache_clear()
