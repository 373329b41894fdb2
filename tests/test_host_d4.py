"""CPU: the D4 yardstick (tests/d4_ref.py) against the index table of include/dsr_hip.h, the host-side validation of the new
entry points (csrc/d4.hip) through the built library, and the argument checks of the Python surface.  Nothing is launched."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import d4_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "deep-super-resolution_amd"
DSR_E_ARG = -1


@pytest.fixture(scope="module")
def so():
    b = importlib.import_module(PKG + "._build")
    return b.build()


def test_transforms_invert_and_are_distinct():
    x = torch.arange(2 * 5 * 7, dtype=torch.float32).reshape(2, 5, 7)
    images = []
    for k in range(8):
        y = d4_ref.T(x, k)
        assert tuple(y.shape) == ((2, 5, 7) if k % 2 == 0 else (2, 7, 5)), k
        assert torch.equal(d4_ref.T_inv(y, k), x), k
        images.append(y)
    sq = torch.arange(36, dtype=torch.float32).reshape(6, 6)        # on a square all eight have one shape: compare them
    turned = [d4_ref.T(sq, k) for k in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not torch.equal(turned[a], turned[b]), (a, b)
            if images[a].shape == images[b].shape:
                assert not torch.equal(images[a], images[b]), (a, b)


@pytest.mark.parametrize("shape", [(5, 7), (1, 4), (3, 1), (1, 1), (2, 6, 6), (2, 130, 67), (1, 65, 129)])
def test_yardstick_agrees_with_the_gather_table(shape):
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    for k in range(8):
        assert torch.equal(d4_ref.T(x, k), d4_ref.gather(x, k)), k


def test_inverse_is_a_group_element():
    """infer.d4_inverse runs T_k^-1 as another T: a quarter turn is undone by the opposite one, a mirrored code by itself."""
    x = torch.arange(35, dtype=torch.float32).reshape(5, 7)
    for k in range(8):
        inv = k if k >= 4 else (4 - k) % 4
        assert torch.equal(d4_ref.T(d4_ref.T(x, k), inv), x), k


def test_ensemble_mean_order_and_scale():
    vals = [torch.tensor([1.0, 1e8, 3.0]), torch.tensor([1e-3, -1e8, 3.0]), torch.tensor([2.0, 0.5, 3.0])]
    got = d4_ref.ensemble_mean([vals[2], vals[0], vals[1]], [7, 0, 3])          # summed as codes 0, 3, 7
    third = np.float32(1.0) / np.float32(3.0)
    want = [np.float32(np.float32(np.float32(a) + np.float32(b)) + np.float32(c)) * third for a, b, c in zip(*[v.tolist() for v in vals])]
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), np.array(want, dtype=np.float32))
    assert got[1].item() == float(np.float32(0.5) * third)                      # (1e8 - 1e8) + 0.5: the order matters


def test_bad_arguments_return_codes_not_crashes(so):
    """Every new entry point validates on the host and returns DSR_E_ARG before anything is launched (no GPU needed)."""
    L = importlib.import_module(PKG + "._lib")
    lib = L.lib()
    N, st = None, None
    one = ctypes.c_void_p(16)            # a non-null "pointer" that is never dereferenced: validation fails first
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    img = (ctypes.c_void_p * 1)(16)
    calls = [
        lambda: lib.dsr_patch_batch_u8_d4(1, None, None, None, None, None, None, 4, 4, 0, N, st),                 # null tables
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(8), I(8), I(0), I(0), None, 4, 4, 0, one, st),                # null xforms
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(8), I(8), I(0), I(0), I(8), 4, 4, 0, one, st),                # code 8
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(8), I(8), I(0), I(0), I(-1), 4, 4, 0, one, st),               # code -1
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(8), I(8), I(0), I(0), I(1), 4, 6, 0, one, st),                # code 1, ph != pw
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(8), I(8), I(0), I(0), I(7), 6, 4, 0, one, st),                # code 7, ph != pw
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(4), I(4), I(2), I(0), I(0), 4, 4, 0, one, st),                # rows 2..5 of 4
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(4), I(4), I(0), I(1), I(2), 4, 4, 0, one, st),                # columns 1..4 of 4
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(4), I(4), I(0), I(0), I(0), 4, 4, 9, one, st),                # mode
        lambda: lib.dsr_patch_batch_u8_d4(1, img, I(4), I(4), I(0), I(0), I(0), 4, 4, 0, N, st),                  # null out
        lambda: lib.dsr_d4_expand_f32(N, 3, 4, 4, 0xFF, one, one, st),                                            # null source
        lambda: lib.dsr_d4_expand_f32(one, 3, 4, 4, 0, one, one, st),                                             # mask 0
        lambda: lib.dsr_d4_expand_f32(one, 3, 4, 4, 0x100, one, one, st),                                         # a ninth code
        lambda: lib.dsr_d4_expand_f32(one, 3, 0, 4, 0xFF, one, one, st),
        lambda: lib.dsr_d4_expand_f32(one, 0, 4, 4, 0xFF, one, one, st),
        lambda: lib.dsr_d4_expand_f32(one, 3, 4, 4, 0x01, N, one, st),                                            # code 0 needs dst_even
        lambda: lib.dsr_d4_expand_f32(one, 3, 4, 4, 0x02, one, N, st),                                            # code 1 needs dst_odd
        lambda: lib.dsr_d4_mean_f32(one, one, 3, 4, 4, 0, one, st),                                               # mask 0
        lambda: lib.dsr_d4_mean_f32(one, one, 3, 4, 4, 0xFF, N, st),                                              # null destination
        lambda: lib.dsr_d4_mean_f32(one, one, 3, 4, -1, 0xFF, one, st),
        lambda: lib.dsr_d4_mean_f32(one, one, 3, 0, 4, 0xFF, one, st),
        lambda: lib.dsr_d4_mean_f32(one, one, 0, 4, 4, 0xFF, one, st),
        lambda: lib.dsr_d4_mean_f32(N, one, 3, 4, 4, 0x04, one, st),                                              # code 2 needs src_even
        lambda: lib.dsr_d4_mean_f32(one, N, 3, 4, 4, 0x80, one, st),                                              # code 7 needs src_odd
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc == DSR_E_ARG, f"call #{i} returned {rc}"
        assert lib.dsr_last_error(), i


def test_patch_bank_validates_transforms_before_device_work():
    """PatchBank.sample / patch_batch refuse a wrong number of codes, a code outside 0..7 and a quarter turn of a non-square
    patch with ValueError, before any image is touched: the bank here holds host tensors, which the launch path rejects."""
    DS = importlib.import_module(PKG + ".dataset")
    lr = torch.zeros((24, 40, 3), dtype=torch.uint8)
    hr = torch.zeros((96, 160, 3), dtype=torch.uint8)
    rng = np.random.RandomState(5)
    state = rng.get_state()[1].copy()
    wide = DS.PatchBank([(lr, hr)], 4, (16, 8), rng=rng)
    square = DS.PatchBank([(lr, hr)], 4, (8, 8), rng=rng, augment=True)
    for bank, n, codes in [(wide, 3, [0, 2]), (wide, 3, [0, 2, 4, 6]), (wide, 2, [0, 8]), (wide, 2, [-1, 0]), (wide, 2, [0, 1]),
                           (wide, 2, [3, 0]), (square, 2, [9, 0]), (square, 2, [1])]:
        with pytest.raises(ValueError):
            bank.sample(n, transforms=codes)
    with pytest.raises(ValueError):
        wide.sample(5, indices=[0, 0], transforms=[0, 2, 4, 6, 0])              # the length follows `indices`
    assert np.array_equal(rng.get_state()[1], state)                            # refused before any draw
    with pytest.raises(ValueError):
        DS.patch_batch([lr], [0], [0], 8, 16, DS.PATCH_UNIT, transforms=[5])
    with pytest.raises(ValueError):
        DS.patch_batch([lr], [0], [0], 8, 8, DS.PATCH_UNIT, transforms=[0, 1])
    with pytest.raises(TypeError):                                              # valid codes: the host image is what stops it
        wide.sample(2, transforms=[0, 6])


def test_infer_validates_codes():
    inf = importlib.import_module(PKG + ".infer")
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError):
        inf.d4(x, 8)
    with pytest.raises(ValueError):
        inf.d4_inverse(x, -1)
    with pytest.raises(TypeError):
        inf.d4(x, 3)                                                            # a host tensor
    with pytest.raises(ValueError):
        inf.super_resolve(None, x, self_ensemble=(0, 8))
    with pytest.raises(ValueError):
        inf.super_resolve(None, x, self_ensemble=())
    with pytest.raises(ValueError):
        inf.super_resolve(None, x, self_ensemble=True, ensemble_batch=0)
