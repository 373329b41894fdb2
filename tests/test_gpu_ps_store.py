"""GPU: the PixelShuffle(2) convolutions (64 -> 256, generator.py:28-39) on conv_c64_kernel with one 64-channel slice per
sub-pixel: slice s = blockIdx.y computes the conv channels {4c + s}, keeps the plain C-tile layout and stores whole 128-byte
output pixels at (2y + sy, 2x + sx).

Exact-grid operands (ternary input and weights, integer bias: every product and sum exact in fp32, every stored value
representable in bf16 and fp16) against float64 conv2d -> pixel_shuffle -> PReLU on the CPU, compared for equality, in both
storage types, in the train form (autograd on) and the inference form (torch.no_grad()).  Both forms reach mode 1 of the
kernel, conv_c64_kernel<1>: the PixelShuffle blocks carry no BatchNorm, and dsr_conv_fwd refuses PixelShuffle together with
the folded epilogue of mode 2, so the inference form differs in what the Python side saves, not in the kernel.  The bias of
conv channel k is k - 128 and the weight rows are pairwise different, so a slice, sub-pixel or channel mix-up cannot cancel.

Shapes (tiles are 4 rows x 32 columns in mode 1; 128 persistent blocks per slice):
  N=1,  5 x 33   ragged in both directions; tiles that touch both image edges
  N=3, 48 x 128  144 tiles per slice: 16 blocks take a second tile (next-tile DMA prefetch, counted outstanding stores)
One random-data case (N=2, 36 x 96, bf16) must equal, bit for bit, the output of the kernel before the slices were re-cut
(32-byte pieces, 64 consecutive conv channels per slice): the products summed into every output element and their order did not
change.  The whole output is 3.4 MiB, beyond the fixture size limit, so tests/golden/ps_store_n2_36x96.npz holds the SHA-256
of its bytes and, for a readable failure, the first and last 8 output rows of image 0 and the last 8 of image 1."""
import functools
import hashlib
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
SLOPE = 0.25
GOLDEN = "ps_store_n2_36x96"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def nhwc(t, tdt, dev):
    out = t.permute(0, 2, 3, 1).contiguous().to(tdt)
    assert torch.equal(out.double(), t.permute(0, 2, 3, 1).double())
    return out.to(dev)


def reference(x, w, b):
    """float64 conv2d -> pixel_shuffle -> PReLU, NCHW."""
    z = TF.pixel_shuffle(TF.conv2d(x.double(), w.double(), b.double(), padding=1), 2)
    return torch.where(z >= 0, z, z * SLOPE)


@functools.lru_cache(maxsize=None)
def exact_case(n, h, w):
    """Operands and the expected output of one exact-grid case; computed once and shared: callers must not modify it."""
    gen = torch.Generator().manual_seed(4200 + 1000 * n + 10 * h + w)
    x = R.ternary(gen, (n, 64, h, w), 0.25)
    wt = R.ternary(gen, (256, 64, 3, 3), 0.25)
    assert len({tuple(r.tolist()) for r in wt.view(256, -1)}) == 256, "weight rows must differ per conv channel"
    b = torch.arange(256, dtype=torch.float64) - 128.0
    y = reference(x, wt, b)
    bound = float(TF.conv2d(x.abs(), wt.abs(), padding=1).max()) + 128.0
    assert bound < R.EXACT_LIMIT
    for dt in (R.BF16, R.F16):
        assert R.representable(y, dt), "the expected output must need no rounding"
    return x, wt, b, y


def conv_act(dev, x, wt, b, tdt, train):
    """functional.ConvAct with PixelShuffle(2) + PReLU; returns (y [N, 2H, 2W, 64] on the device, forward kernel name)."""
    F = P("functional")
    log = []
    old, F.KERNEL_LOG = F.KERNEL_LOG, log
    try:
        xg = nhwc(x, tdt, dev).requires_grad_(train)
        wg = wt.float().to(dev).requires_grad_(train)
        bg = b.float().to(dev).requires_grad_(train)
        ag = torch.full((1,), SLOPE, device=dev, requires_grad=train)
        cfg = dict(stride=1, pad=1, act=F.ACT_PRELU, pixel_shuffle=True)
        if train:
            y = F.ConvAct.apply(xg, wg, bg, ag, cfg)
            assert y.requires_grad
        else:
            with torch.no_grad():
                y = F.ConvAct.apply(xg, wg, bg, ag, cfg)
        torch.cuda.synchronize()
    finally:
        F.KERNEL_LOG = old
    names = [e[4] for e in log if e[0] == "fwd"]
    return y.detach(), names


def same(got, want, what):
    got, want = got.double().cpu(), want.double()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ; first at {bad[:6].tolist()}: got "
                             f"{got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")


@pytest.mark.parametrize("train", [True, False], ids=["train", "no_grad"])
@pytest.mark.parametrize("dtype", [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")])
@pytest.mark.parametrize("n,h,w", [(1, 5, 33), (3, 48, 128)])
def test_pixel_shuffle_slices_exact(dev, n, h, w, dtype, train):
    """Every output element equals the float64 reference; the launch is conv_c64_kernel<1>."""
    x, wt, b, want = exact_case(n, h, w)
    y, names = conv_act(dev, x, wt, b, R.DTYPES[dtype], train)
    assert names == ["conv_c64_kernel<1>"], names
    assert tuple(y.shape) == (n, 2 * h, 2 * w, 64)
    same(y.permute(0, 3, 1, 2), want, "y (pixel shuffle)")


def random_case():
    """N=2, 36 x 96, bf16: operands of the saved-output case (seeded CPU generator; values rounded to bf16 first)."""
    gen = torch.Generator().manual_seed(20260)
    x = torch.randn((2, 64, 36, 96), generator=gen).bfloat16().float()
    wt = (torch.randn((256, 64, 3, 3), generator=gen) * float(np.sqrt(2.0 / 576))).bfloat16().float()
    b = (torch.randn((256,), generator=gen) * 0.1).float()
    return x, wt, b


def golden_crops(y):
    """y: [2, 72, 192, 64] int16 view of the bf16 output (numpy)."""
    return dict(n0_top=y[0, :8], n0_bottom=y[0, -8:], n1_bottom=y[1, -8:])


def test_random_case_equals_the_saved_output(dev, golden):
    """Bit identity with the kernel that stored 32-byte pieces (file docstring).  Prints the deviation from the fp32
    reference on the way: it is that kernel's own, by construction."""
    x, wt, b = random_case()
    y, names = conv_act(dev, x, wt, b, torch.bfloat16, False)
    assert names == ["conv_c64_kernel<1>"], names
    ref = reference(x, wt, b).permute(0, 2, 3, 1)
    err = (y.double().cpu() - ref).abs()
    print(f"vs float64 reference: max |diff| {err.max().item():.4e}, relative to max |ref| {err.max().item() / ref.abs().max().item():.4e}")
    bits = y.cpu().contiguous().view(torch.int16).numpy()
    g = golden(GOLDEN)
    assert tuple(g["shape"]) == bits.shape
    for k, v in golden_crops(bits).items():
        assert np.array_equal(v, g[k]), f"{k}: {int((v != g[k]).sum())} of {v.size} stored values differ from the saved output"
    assert hashlib.sha256(bits.tobytes()).hexdigest() == str(g["sha256"]), "the output differs from the saved one outside the crops"
