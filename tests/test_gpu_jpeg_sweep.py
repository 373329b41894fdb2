"""GPU: the JPEG round trip (csrc/jpeg.hip) past the regimes tests/test_gpu_jpeg.py runs it in, BIT FOR BIT against
tests/jpeg_ref.py (which tests/test_host_jpeg.py holds to Pillow at every size and quality used here).  No tolerance anywhere.

1. every quality 1..100 (the tables and the float-reciprocal quantiser are derived per quality in the kernel);
2. the chroma half of jpeg420_planes_kernel past its first thread block of 32 chroma blocks, and the corners of upsample4:
   replication with a chroma width of 2, the triangle filter with a chroma height of 1;
3. the raw ABI between sentinel margins: `out`, and a 4:2:0 workspace of exactly dsr_jpeg_workspace bytes;
4. dsr_jpeg_batch_f32 in all four scalings at the widths where F32Batch mixes its 16-byte and scalar paths, and off alignment."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import jpeg_ref
from test_gpu_jpeg import QUALITIES, pictures, ref

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
MARGIN = 512                                                           # elements on each side: a multiple of 16 bytes in both types


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view({1: torch.uint8, 4: torch.int32}[t.element_size()])


class Guard:
    """Device buffers between MARGIN sentinel elements on each side, `skew` elements further into the allocation; check()
    asserts that every margin kept its bits."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, numel, dtype, fill, margin, skew=0):
        flat = torch.full((skew + numel + 2 * MARGIN,), margin, dtype=dtype, device=self.dev)[skew:]
        flat[MARGIN:MARGIN + numel] = fill
        self.bufs.append((flat, _bits(flat[:MARGIN]).clone(), _bits(flat[MARGIN + numel:]).clone(), numel))
        return flat[MARGIN:MARGIN + numel]

    def put(self, t, margin, skew=0):
        v = self.new(t.numel(), t.dtype, 0, margin, skew).view(t.shape)
        v.copy_(t)
        return v

    def check(self):
        torch.cuda.synchronize()
        for flat, lo, hi, numel in self.bufs:
            assert torch.equal(_bits(flat[:MARGIN]), lo) and torch.equal(_bits(flat[MARGIN + numel:]), hi), "write outside a buffer"


@functools.lru_cache(maxsize=None)
def quality_batch(h, w):
    """(uint8 [200, h, w, 3], the 200 qualities): a noise and a saturated 0 / 255 picture, each at q = 1..100."""
    rng = np.random.RandomState(1000 * h + w)
    noise = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    sat = (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    imgs = np.stack([noise] * 100 + [sat] * 100)
    imgs.setflags(write=False)
    return imgs, list(range(1, 101)) * 2


# ============================================================================= 1. every quality
@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("size", [(16, 16), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_quality(dev, size, subsampling):
    """make_tables and the quantiser of codec_block at every q in 1..100 (5000 / q below 50, 200 - 2 q from there; the float
    reciprocal of each of the 2 x 64 divisors 8 t, corrected by one step), one batch of 200 with a quality per sample."""
    D = P("utils.degradation")
    imgs, qs = quality_batch(*size)
    got = D.jpeg_compress(torch.from_numpy(imgs.copy()).to(dev), qs, subsampling).cpu().numpy()
    bad = [("noise" if n < 100 else "saturated", qs[n]) for n in range(200) if not np.array_equal(got[n], ref(imgs[n], qs[n], subsampling))]
    assert not bad, f"(picture, quality) that differ: {bad}"


# ============================================================================= 2. past one chroma group; the corners of upsample4
# (81, 97): 11 x 13 = 143 luma blocks in 5 groups of 32, the last holding 15; chroma 41 x 49 -> 6 x 7 = 42 blocks in 2 groups, the
# last holding 10.  (128, 128): 256 luma and 64 chroma blocks, 8 and 2 full groups: no `want >= nblk` guard fires.  (64, 144):
# 4 x 9 = 36 chroma blocks.  (9, 4), (9, 3): chroma width 2, replication with both columns read.  (1, 9), (2, 17): chroma height 1
# with widths 5 and 9, the triangle filter whose neighbour row is the row itself.
# (tests/test_host_jpeg.py::test_sweep_sizes_cross_what_they_claim counts the blocks)
SWEEP_SIZES = [(81, 97), (128, 128), (64, 144), (9, 4), (9, 3), (1, 9), (2, 17)]


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("size", SWEEP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_past_one_chroma_group(dev, size, subsampling):
    """The seven pictures of test_gpu_jpeg.py at its four qualities as one batch of 28."""
    D = P("utils.degradation")
    h, w = size
    imgs = [im for im in pictures(h, w, 100 * h + w) for _ in QUALITIES]
    qs = list(QUALITIES) * 7
    got = D.jpeg_compress(torch.from_numpy(np.stack(imgs)).to(dev), qs, subsampling).cpu().numpy()
    bad = [(n // 4, qs[n]) for n in range(len(imgs)) if not np.array_equal(got[n], ref(imgs[n], qs[n], subsampling))]
    assert not bad, f"(picture, quality) that differ: {bad}"


# ============================================================================= 3. the raw ABI between margins
MARGIN_QS = (7, 60, 93)


def _workspace(g, lib, n, h, w, ss):
    size = lib.dsr_jpeg_workspace(n, h, w, ss)
    if ss == 0:
        assert size == 0
        return None
    hy, wy, hc, wc = (h + 7) // 8 * 8, (w + 7) // 8 * 8, ((h + 1) // 2 + 7) // 8 * 8, ((w + 1) // 2 + 7) // 8 * 8
    assert size == n * (hy * wy + 2 * hc * wc)
    ws = g.new(size, torch.uint8, 0x5A, 0xA5)
    assert ws.data_ptr() % 16 == 0
    return ws


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("size", [(81, 97), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_u8_between_margins(dev, size, subsampling):
    """dsr_jpeg_u8, count 3: `out` pre-filled with 0x00 and then with 0xFF (a byte that is never stored cannot be the
    yardstick's both times) between margins of 0xA5, the 4:2:0 workspace exactly dsr_jpeg_workspace bytes between margins."""
    L = P("_lib")
    lib = L.lib()
    h, w = size
    imgs = pictures(h, w, 7 * h + w)[:3]
    want = np.stack([ref(imgs[n], MARGIN_QS[n], subsampling) for n in range(3)])
    for fill in (0x00, 0xFF):
        g = Guard(dev)
        src = g.put(torch.from_numpy(np.stack(imgs)).to(dev), 0xA5)
        q = g.put(torch.tensor(MARGIN_QS, dtype=torch.int32, device=dev), 50)
        out = g.new(3 * h * w * 3, torch.uint8, fill, 0xA5).view(3, h, w, 3)
        ws = _workspace(g, lib, 3, h, w, subsampling)
        L.check(lib.dsr_jpeg_u8(_ptr(src), _ptr(out), 3, h, w, _ptr(q), subsampling, None if ws is None else _ptr(ws), _st()))
        g.check()
        assert np.array_equal(out.cpu().numpy(), want), fill
        assert np.array_equal(src.cpu().numpy(), np.stack(imgs)) and q.tolist() == list(MARGIN_QS)


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("size", [(81, 97), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_f32_between_margins(dev, size, subsampling):
    """dsr_jpeg_batch_f32, count 3: `out` pre-filled with NaN between NaN margins, the input between NaN margins (a read past
    an end would reach the levels), the workspace as above."""
    L = P("_lib")
    lib = L.lib()
    h, w = size
    imgs = pictures(h, w, 7 * h + w)[:3]
    want = jpeg_ref.scale_f32(np.stack([ref(imgs[n], MARGIN_QS[n], subsampling) for n in range(3)]), jpeg_ref.UNIT)
    x = torch.from_numpy(jpeg_ref.scale_f32(np.stack(imgs), jpeg_ref.UNIT))
    assert np.array_equal(jpeg_ref.levels_f32(x.numpy()), np.stack(imgs))
    g = Guard(dev)
    src = g.put(x.to(dev), float("nan"))
    q = g.put(torch.tensor(MARGIN_QS, dtype=torch.int32, device=dev), 50)
    out = g.new(3 * 3 * h * w, torch.float32, float("nan"), float("nan")).view(3, 3, h, w)
    ws = _workspace(g, lib, 3, h, w, subsampling)
    L.check(lib.dsr_jpeg_batch_f32(_ptr(src), _ptr(out), 3, h, w, _ptr(q), subsampling, 0, None if ws is None else _ptr(ws), _st()))
    g.check()
    assert np.array_equal(out.cpu().numpy(), want)


# ============================================================================= 4. fp32 batches: every scaling, mixed paths
# F32Batch takes 16-byte vectors where a run lies inside the row, starts on a 16-byte boundary and the plane is a multiple of 4
# elements.  (20, 24): all vector.  (18, 20): W % 8 == 4, the last block of a row and the second 16-pixel chroma load go scalar,
# the rest is vector.  (16, 34): W = 2 mod 4, even rows vector, odd rows scalar.  (17, 34): the plane is no multiple of 4, all
# scalar.  (17, 33): odd on both axes.  skew 1: `in` and `out` one float into their allocations, 4 bytes off alignment.
F32_CASES = [((20, 24), 0), ((18, 20), 0), ((16, 34), 0), ((17, 34), 0), ((17, 33), 0), ((20, 24), 1)]
F32_QS = (10, 50, 90, 100)


@functools.lru_cache(maxsize=None)
def f32_inputs(h, w):
    """fp32 [4, 3, h, w], read only: values off the grey levels and outside [0, 1]."""
    f = (torch.rand((4, 3, h, w), generator=torch.Generator().manual_seed(100 * h + w)) * 1.2 - 0.1).to(torch.float32)
    levels = jpeg_ref.levels_f32(f.numpy())
    assert levels.min() == 0 and levels.max() == 255 and float(f.min()) < 0 and float(f.max()) > 1
    levels.setflags(write=False)
    return f, levels


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["UNIT", "LR_REF", "HR_REF", "HR_UNIT"])
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}" + ("-skewed" if c[1] else ""))
def test_f32_batch_every_scaling_and_path(dev, case, mode, subsampling):
    L = P("_lib")
    lib = L.lib()
    (h, w), skew = case
    f, levels = f32_inputs(h, w)
    want = jpeg_ref.scale_f32(np.stack([ref(levels[n], F32_QS[n], subsampling) for n in range(4)]), mode)
    g = Guard(dev)
    src = g.put(f.to(dev), float("nan"), skew)
    out = g.new(f.numel(), torch.float32, float("nan"), float("nan"), skew).view(4, 3, h, w)
    assert src.data_ptr() % 16 == 4 * skew and out.data_ptr() % 16 == 4 * skew
    q = torch.tensor(F32_QS, dtype=torch.int32, device=dev)
    size = lib.dsr_jpeg_workspace(4, h, w, subsampling)
    ws = g.new(size, torch.uint8, 0x5A, 0xA5) if size else None
    L.check(lib.dsr_jpeg_batch_f32(_ptr(src), _ptr(out), 4, h, w, _ptr(q), subsampling, mode, None if ws is None else _ptr(ws), _st()))
    g.check()
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(src.cpu(), f)
