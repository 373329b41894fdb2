"""GPU: utils.degradation.filter2d (csrc/filter2d.hip) against the float64 yardstick tests/filter2d_ref.py.

Exact sweep: data k / 256 and dyadic kernels (integers in -8..8 over 64).  Every product is a multiple of 2^-14 and every
partial sum of at most 441 of them stays below 56, i.e. needs 6 + 14 = 20 bits: nothing rounds in fp32, the summation order
cannot show, and the comparison is ==.  Float kernels: the derived bound (ks^2 + 2) 2^-24 sum|k| max|x| (filter2d_ref.bound)."""
import importlib

import numpy as np
import pytest
import torch

import filter2d_ref as FR

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
SHAPES = [(3, 3, 11, 11), (2, 1, 37, 19), (1, 4, 70, 131)]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def _data(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed)).float() / 256.0


def _dyadic(n, ks, seed):
    return torch.randint(-8, 9, (n, ks, ks), generator=torch.Generator().manual_seed(seed)).float() / 64.0


@pytest.mark.parametrize("ks", [1, 3, 7, 21])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_sweep(dev, shape, ks):
    D = P("utils.degradation")
    x = _data(shape, ks + shape[2])
    k = _dyadic(shape[0], ks, 100 + ks)
    want = FR.filter2d(x, k)
    got = D.filter2d(x.to(dev), k.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert torch.equal(got.cpu().double(), want)
    # one kernel for all samples
    want_s = FR.filter2d(x, k[0])
    assert torch.equal(D.filter2d(x.to(dev), k[0].to(dev)).cpu().double(), want_s)
    assert torch.equal(want_s, want) == bool((k == k[0]).all())            # (the per-sample kernels do differ, 1 x 1 by chance aside)
    # numpy kernels are uploaded
    assert torch.equal(D.filter2d(x.to(dev), k.numpy()).cpu().double(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_padded_kernel_gives_the_bits_of_the_kernel(dev, shape):
    """7 x 7 inside 21 x 21: the kernel skips the zero tap rows and columns; the bits are those of the 7 x 7 call, for dyadic and
    for float kernels (the 7 x 7 call itself is held to the yardstick by the exact sweep)."""
    D = P("utils.degradation")
    x = _data(shape, 5).to(dev)
    for k7 in (_dyadic(shape[0], 7, 6), torch.from_numpy(D.random_mixed_kernels(shape[0], size=7, sinc_prob=0.5, pad_to=7,
                                                                                rng=np.random.RandomState(2)))):
        k21 = torch.zeros(shape[0], 21, 21)
        k21[:, 7:14, 7:14] = k7
        small, padded = D.filter2d(x, k7.to(dev)), D.filter2d(x, k21.to(dev))
        assert torch.equal(small, padded)
    # an off-centre support (rows 2..4, columns 17..20) and an all-zero kernel
    odd = torch.zeros(shape[0], 21, 21)
    odd[:, 2:5, 17:21] = _dyadic(shape[0], 21, 9)[:, 2:5, 17:21]
    assert torch.equal(D.filter2d(x, odd.to(dev)).cpu().double(), FR.filter2d(x.cpu(), odd))
    assert not bool(D.filter2d(x, torch.zeros(shape[0], 21, 21, device=dev)).any())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_kernels_within_the_derived_bound(dev, shape):
    D = P("utils.degradation")
    k = torch.from_numpy(D.random_mixed_kernels(shape[0], size=tuple(range(7, 22, 2)), sinc_prob=0.4, rng=np.random.RandomState(shape[3])))
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    want = FR.filter2d(x, k)
    got = D.filter2d(x.to(dev), k.to(dev)).cpu().double()
    err, bound = float((got - want).abs().max()), FR.bound(k, x)
    print(f"filter2d {shape}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_a_window_does_not_depend_on_the_tiles_that_reach_it(dev):
    """The 70 x 131 image, and the same pixels as the lower right part of another batch: sample 1 of 2, three planes instead of
    four, cut at (5, 9) so that every tile border moves.  Away from the new top and left borders (r = 10 pixels) the two runs
    see the same neighbourhoods (the bottom and right borders reflect alike) and must agree bit for bit."""
    D = P("utils.degradation")
    x = torch.rand((1, 4, 70, 131), generator=torch.Generator().manual_seed(3))
    k = torch.from_numpy(D.random_mixed_kernels(1, size=21, sinc_prob=1.0, rng=np.random.RandomState(4)))
    full = D.filter2d(x.to(dev), k.to(dev))
    other = torch.rand((2, 3, 65, 122), generator=torch.Generator().manual_seed(5))
    other[1] = x[0, 1:4, 5:, 9:]
    k2 = torch.cat([torch.from_numpy(D.random_mixed_kernels(1, rng=np.random.RandomState(6))), k])
    moved = D.filter2d(other.to(dev), k2.to(dev))
    assert torch.equal(moved[1, :, 10:, 10:], full[0, 1:4, 15:, 19:])
    assert not torch.equal(moved[1, :, :10, :], full[0, 1:4, 5:15, 9:])


def test_refused_arguments_launch_nothing(dev):
    D, L, Fn = P("utils.degradation"), P("_lib"), P("functional")
    lib = L.lib()
    x = torch.rand(1, 3, 10, 32, device=dev)
    y = torch.full_like(x, -7.0)
    k = torch.rand(1, 23, 23, device=dev)
    st = Fn._stream()
    p = Fn._ptr
    assert lib.dsr_filter2d_f32(p(x), p(y), p(k), 1, 3, 10, 32, 21, 0, st) == -1            # H = 10, ks = 21
    assert lib.dsr_filter2d_f32(p(x), p(y), p(k), 1, 3, 10, 32, 8, 0, st) == -1             # even
    assert lib.dsr_filter2d_f32(p(x), p(y), p(k), 1, 3, 10, 32, 23, 0, st) == -1            # > 21
    assert lib.dsr_filter2d_f32(p(x), p(x), p(k), 1, 3, 10, 32, 3, 0, st) == -1             # y == x
    assert b"overlaps" in lib.dsr_last_error()
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    for bad in (lambda: D.filter2d(x, k), lambda: D.filter2d(x, torch.rand(1, 8, 8, device=dev)),
                lambda: D.filter2d(x, torch.rand(1, 21, 21, device=dev)), lambda: D.filter2d(x, torch.rand(2, 3, 3, device=dev))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        D.filter2d(x.half(), torch.rand(1, 3, 3, device=dev))
