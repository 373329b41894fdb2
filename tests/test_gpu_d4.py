"""GPU: the D4 kernels (csrc/d4.hip) and what is built on them -- PatchBank augmentation and geometric self-ensemble inference
-- against tests/d4_ref.py (torch.flip / torch.rot90 on the CPU; tests/test_host_d4.py checks that yardstick itself).

The kernels move values and add them in a fixed order, so everything up to the generator is compared BIT FOR BIT; the
batched fp16 ensemble is held to the bound a single fp16 forward is held to (0.02, test_generator_fp16_inference), the tiled
one to the 2e-3 of test_tiled_inference_matches_whole_image."""
import copy
import ctypes
import importlib
import zlib

import numpy as np
import pytest
import torch

import d4_ref
from oracle import filler, gan, losses

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
SENTINEL = -12345.0
GUARD = 67
SHAPES = [(3, 37, 70), (2, 64, 64), (1, 1, 5), (1, 5, 1), (1, 1, 1),      # (planes, h, w)
          (2, 130, 67), (1, 65, 129)]      # 3 x 2 and 2 x 3 tiles of 64 x 64, ragged on both axes: tile rows with a0 > 0


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    P("_lib").lib()
    return torch.device("cuda:0")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, dev):
    """a flat fp32 device buffer of n elements followed by GUARD sentinels (the whole buffer starts as sentinels)"""
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)


def random_image(tag, shape):
    rng = np.random.RandomState(zlib.crc32(tag.encode()))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------ dsr_d4_expand_f32
@pytest.mark.parametrize("planes,h,w", SHAPES)
def test_expand_bit_equal_to_the_yardstick(dev, planes, h, w):
    L = P("_lib")
    x = random_image(f"expand{planes}x{h}x{w}", (planes, h, w))
    xd = x.to(dev)
    n = planes * h * w
    for mask in [0xFF, 0x55, 0xAA] + [1 << k for k in range(8)]:
        codes = d4_ref.codes_of(mask)
        even, odd = [k for k in codes if k % 2 == 0], [k for k in codes if k % 2]
        de, do = guarded(len(even) * n, dev), guarded(len(odd) * n, dev)
        L.check(L.lib().dsr_d4_expand_f32(ptr(xd), planes, h, w, mask, ptr(de) if even else None, ptr(do) if odd else None, stream()))
        de, do = de.cpu(), do.cpu()
        for s, k in enumerate(even):
            assert torch.equal(de[s * n:(s + 1) * n].reshape(planes, h, w), d4_ref.T(x, k)), (hex(mask), k)
        for s, k in enumerate(odd):
            assert torch.equal(do[s * n:(s + 1) * n].reshape(planes, w, h), d4_ref.T(x, k)), (hex(mask), k)
        assert bool((de[len(even) * n:] == SENTINEL).all()) and bool((do[len(odd) * n:] == SENTINEL).all()), hex(mask)
    assert torch.equal(xd.cpu(), x)                                      # the source is not written


def test_d4_and_inverse_surface(dev):
    inf = P("infer")
    x = random_image("surface", (2, 3, 9, 13))
    xd = x.to(dev)
    for k in range(8):
        y = inf.d4(xd, k)
        assert tuple(y.shape) == ((2, 3, 9, 13) if k % 2 == 0 else (2, 3, 13, 9)) and y.dtype == torch.float32
        assert torch.equal(y.cpu(), d4_ref.T(x, k)), k
        assert torch.equal(inf.d4_inverse(y, k).cpu(), x), k
        assert torch.equal(inf.d4_inverse(xd, k).cpu(), d4_ref.T_inv(x, k)), k


# ------------------------------------------------------------------ dsr_d4_mean_f32
@pytest.mark.parametrize("planes,h,w", SHAPES)
def test_mean_bit_equal_to_the_yardstick(dev, planes, h, w):
    """Eight DIFFERENT random tensors (not transforms of one image, which would hide a wrong slot or a wrong order); values of
    mixed magnitude so that a different summation order rounds differently."""
    L = P("_lib")
    srcs = []
    for k in range(8):
        shape = (planes, h, w) if k % 2 == 0 else (planes, w, h)
        srcs.append(random_image(f"mean{k}:{planes}x{h}x{w}", shape) * float(10.0 ** (k % 3)))
    n = planes * h * w
    for mask in [0xFF, 0x0F, 0xA0, 0x07, 0x10]:
        codes = d4_ref.codes_of(mask)
        even, odd = [k for k in codes if k % 2 == 0], [k for k in codes if k % 2]
        se = torch.stack([srcs[k] for k in even]).to(dev) if even else None
        so = torch.stack([srcs[k] for k in odd]).to(dev) if odd else None
        dst = guarded(n, dev)
        L.check(L.lib().dsr_d4_mean_f32(ptr(se) if even else None, ptr(so) if odd else None, planes, h, w, mask, ptr(dst), stream()))
        dst = dst.cpu()
        want = d4_ref.ensemble_mean([d4_ref.T_inv(srcs[k], k) for k in codes], codes)
        assert tuple(want.shape) == (planes, h, w)
        got = dst[:n].reshape(planes, h, w)
        assert torch.equal(got, want), (hex(mask), float((got - want).abs().max()))
        assert bool((dst[n:] == SENTINEL).all()), hex(mask)


# ------------------------------------------------------------------ patch_batch(transforms=)
@pytest.fixture(scope="module")
def u8_images(dev):
    rng = np.random.RandomState(17)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for h, w in [(41, 53), (64, 64), (50, 47)]]


def _patch_case(u8_images, count, ph, pw, codes, seed):
    rng = np.random.RandomState(seed)
    images, tops, lefts = [], [], []
    for b in range(count):
        im = u8_images[b % 3]
        images.append(im)
        tops.append(int(rng.randint(0, im.shape[0] - ph + 1)))
        lefts.append(int(rng.randint(0, im.shape[1] - pw + 1)))
    # a patch touching its image's last row and last column, one at the origin
    tops[1], lefts[1] = images[1].shape[0] - ph, images[1].shape[1] - pw
    tops[2], lefts[2] = 0, 0
    tops[3], lefts[3] = images[3].shape[0] - ph, images[3].shape[1] - pw
    return images, tops, lefts, [codes[b % len(codes)] for b in range(count)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_patch_batch_transforms_square(dev, u8_images, mode):
    """70 patches of 16 x 16 (two chunks of the 64-entry table), codes cycling 0..7: T_k of the un-transformed launch's patch,
    which tests/test_gpu_data.py pins to the reference."""
    DS = P("dataset")
    images, tops, lefts, codes = _patch_case(u8_images, 70, 16, 16, list(range(8)), 3)
    base = DS.patch_batch(images, tops, lefts, 16, 16, mode).cpu()
    got = DS.patch_batch(images, tops, lefts, 16, 16, mode, transforms=codes).cpu()
    assert tuple(got.shape) == (70, 3, 16, 16)
    for b in range(70):
        assert torch.equal(got[b], d4_ref.T(base[b], codes[b])), (b, codes[b])


def test_patch_batch_transforms_other_shapes(dev, u8_images):
    """12 x 20 patches with the four shape-preserving codes, a whole 64 x 64 image (exactly one tile) under all eight, and a
    quarter turn of a non-square patch refused."""
    DS = P("dataset")
    images, tops, lefts, codes = _patch_case(u8_images, 9, 12, 20, [0, 2, 4, 6], 4)
    for mode in (DS.PATCH_UNIT, DS.PATCH_HR_REF):
        base = DS.patch_batch(images, tops, lefts, 12, 20, mode).cpu()
        got = DS.patch_batch(images, tops, lefts, 12, 20, mode, transforms=codes).cpu()
        for b in range(9):
            assert torch.equal(got[b], d4_ref.T(base[b], codes[b])), (b, codes[b])
    whole = u8_images[1]
    base = DS.patch_batch([whole] * 8, [0] * 8, [0] * 8, 64, 64, DS.PATCH_HR_UNIT).cpu()
    got = DS.patch_batch([whole] * 8, [0] * 8, [0] * 8, 64, 64, DS.PATCH_HR_UNIT, transforms=list(range(8))).cpu()
    for k in range(8):
        assert torch.equal(got[k], d4_ref.T(base[k], k)), k
    with pytest.raises(ValueError):
        DS.patch_batch(images, tops, lefts, 12, 20, DS.PATCH_UNIT, transforms=[1] * 9)


def test_patch_batch_transforms_many_tiles(dev):
    """A 150 x 150 patch of a 160 x 170 image: 3 x 3 tiles of 64 with edge tiles in both directions, all eight codes."""
    DS = P("dataset")
    rng = np.random.RandomState(23)
    im = torch.from_numpy(rng.randint(0, 256, (160, 170, 3), dtype=np.uint8)).to(dev)
    base = DS.patch_batch([im] * 8, [10] * 8, [20] * 8, 150, 150, DS.PATCH_LR_REF).cpu()
    got = DS.patch_batch([im] * 8, [10] * 8, [20] * 8, 150, 150, DS.PATCH_LR_REF, transforms=list(range(8))).cpu()
    for k in range(8):
        assert torch.equal(got[k], d4_ref.T(base[k], k)), k
    wide = DS.patch_batch([im] * 4, [3] * 4, [1] * 4, 70, 130, DS.PATCH_UNIT).cpu()
    got = DS.patch_batch([im] * 4, [3] * 4, [1] * 4, 70, 130, DS.PATCH_UNIT, transforms=[0, 2, 4, 6]).cpu()
    for s, k in enumerate([0, 2, 4, 6]):
        assert torch.equal(got[s], d4_ref.T(wide[s], k)), k


# ------------------------------------------------------------------ PatchBank
@pytest.fixture(scope="module")
def bank_pairs(dev):
    rng = np.random.RandomState(29)
    pairs = []
    for h, w in [(24, 40), (28, 48), (32, 56)]:
        pairs.append((torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev),
                      torch.from_numpy(rng.randint(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8)).to(dev)))
    return pairs


def _draw(pairs, patch, scale, batch, seed):
    """the draws of PatchBank.sample, restated: all indices, then the coordinates; returns the generator for what follows"""
    DS = P("dataset")
    rng = np.random.RandomState(seed)
    idx = [int(rng.randint(0, len(pairs))) for _ in range(batch)]
    coords = [DS.train_patch_coords(pairs[i][0].shape[0], pairs[i][0].shape[1], patch, scale, rng) for i in idx]
    return rng, idx, coords


@pytest.mark.parametrize("patch", [(16, 16), (16, 8)])
def test_patch_bank_augmentation(dev, bank_pairs, patch):
    DS = P("dataset")
    pw, ph = patch
    batch, seed = 12, 41
    rng, idx, coords = _draw(bank_pairs, patch, 4, batch, seed)
    want_lr = DS.patch_batch([bank_pairs[i][0] for i in idx], [c[0] for c in coords], [c[1] for c in coords], ph, pw, DS.PATCH_LR_REF)
    want_hr = DS.patch_batch([bank_pairs[i][1] for i in idx], [c[2] for c in coords], [c[3] for c in coords], 4 * ph, 4 * pw,
                             DS.PATCH_HR_REF)
    # augment=False: the same draws and the same bits as before
    plain_rng = np.random.RandomState(seed)
    lr0, hr0 = DS.PatchBank(bank_pairs, 4, patch, rng=plain_rng).sample(batch)
    assert torch.equal(lr0, want_lr) and torch.equal(hr0, want_hr)
    assert plain_rng.randint(0, 1 << 30) == copy.deepcopy(rng).randint(0, 1 << 30)      # and nothing drawn beyond them
    # augment=True: the same crops, each turned by the code drawn AFTER all coordinates, LR and HR alike
    if pw == ph:
        codes = [int(rng.randint(0, 8)) for _ in range(batch)]
    else:
        codes = [2 * int(rng.randint(0, 4)) for _ in range(batch)]
    lr1, hr1 = DS.PatchBank(bank_pairs, 4, patch, rng=np.random.RandomState(seed), augment=True).sample(batch)
    assert tuple(lr1.shape) == (batch, 3, ph, pw) and tuple(hr1.shape) == (batch, 3, 4 * ph, 4 * pw)
    for b in range(batch):
        assert torch.equal(lr1[b].cpu(), d4_ref.T(want_lr[b].cpu(), codes[b])), (b, codes[b])
        assert torch.equal(hr1[b].cpu(), d4_ref.T(want_hr[b].cpu(), codes[b])), (b, codes[b])
    assert all(k % 2 == 0 for k in codes) or pw == ph
    if pw == ph:
        assert len(set(codes)) > 2 and any(k % 2 for k in codes)           # the seed does exercise the quarter turns
    # explicit codes override the draw, with and without augment
    explicit = [(2 * b) % 8 for b in range(batch)]
    for augment in (False, True):
        lr2, hr2 = DS.PatchBank(bank_pairs, 4, patch, rng=np.random.RandomState(seed), augment=augment).sample(batch, transforms=explicit)
        for b in range(batch):
            assert torch.equal(lr2[b].cpu(), d4_ref.T(want_lr[b].cpu(), explicit[b]))
            assert torch.equal(hr2[b].cpu(), d4_ref.T(want_hr[b].cpu(), explicit[b]))


def test_patch_bank_nonsquare_only_keeps_shape(dev, bank_pairs):
    """Over many draws a non-square bank only ever uses 0, 2, 4, 6 (and uses all four): seen through the output, which has to
    equal one of the four shape-preserving images of the un-augmented crop."""
    DS = P("dataset")
    patch, batch, seed = (16, 8), 48, 7
    rng, idx, coords = _draw(bank_pairs, patch, 4, batch, seed)
    base = DS.patch_batch([bank_pairs[i][0] for i in idx], [c[0] for c in coords], [c[1] for c in coords], 8, 16, DS.PATCH_LR_REF).cpu()
    lr, hr = DS.PatchBank(bank_pairs, 4, patch, rng=np.random.RandomState(seed), augment=True).sample(batch)
    assert tuple(lr.shape) == (batch, 3, 8, 16) and tuple(hr.shape) == (batch, 3, 32, 64)
    seen = set()
    for b in range(batch):
        match = [k for k in (0, 2, 4, 6) if torch.equal(lr[b].cpu(), d4_ref.T(base[b], k))]
        assert match, b
        seen.update(match[:1])
    assert seen == {0, 2, 4, 6}


# ------------------------------------------------------------------ self-ensemble
LR_SHAPES = [(1, 3, 20, 12), (1, 3, 16, 16)]


@pytest.fixture(scope="module")
def ensemble(dev):
    """Generator(4, 2) filled as tests/test_gpu_generator.py::build does, the two LR inputs, and the CPU oracle's fp32 ensemble
    (computed once; nothing below writes to it)."""
    gen = P("models.GAN.generator")
    sd = filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2)))
    g = gen.Generator(4, 2)
    g.load_state_dict(sd)
    g.to(dev)
    lrs, oracle = [], []
    for shape in LR_SHAPES:
        lr = filler.tensor(f"in:d4_ens{shape[2]}x{shape[3]}", shape, 0.5, 0.5)
        outs = []
        with torch.no_grad():
            for k in range(8):
                sr = gan.generator_forward({n: v.clone() for n, v in sd.items()}, d4_ref.T(lr, k), False)
                outs.append(d4_ref.T_inv(sr, k))
        lrs.append(lr)
        oracle.append(outs)
    return g, sd, lrs, oracle


@pytest.mark.parametrize("which", [0, 1])
def test_self_ensemble_exact_path(dev, ensemble, which):
    """ensemble_batch=1: each copy gets the launches of a plain super_resolve of it, so the result IS the yardstick's mean of
    the eight separately super-resolved, turned-back copies -- bit for bit."""
    inf = P("infer")
    g, _, lrs, _ = ensemble
    lr = lrs[which]
    g.train()
    outs = [d4_ref.T_inv(inf.super_resolve(g, d4_ref.T(lr, k).to(dev)).cpu(), k) for k in range(8)]
    want = d4_ref.ensemble_mean(outs, list(range(8)))
    got = inf.super_resolve(g, lr.to(dev), self_ensemble=True, ensemble_batch=1)
    assert tuple(got.shape) == (1, 3, 4 * lr.shape[2], 4 * lr.shape[3]) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    assert g.training and g.compute_dtype == torch.bfloat16                 # mode and dtype restored
    g.eval()
    inf.super_resolve(g, lr.to(dev), self_ensemble=True)
    assert not g.training and g.compute_dtype == torch.bfloat16
    # two codes: the image and its mirror
    want2 = d4_ref.ensemble_mean([outs[0], outs[4]], [0, 4])
    got2 = inf.super_resolve(g, lr.to(dev), self_ensemble=(4, 0), ensemble_batch=1)
    assert torch.equal(got2.cpu(), want2)
    # a batch of two images is two ensembles
    pair = torch.cat([lr, d4_ref.T(lr, 2)]).to(dev)
    got3 = inf.super_resolve(g, pair, self_ensemble=(1, 6), ensemble_batch=1)
    first = d4_ref.ensemble_mean([outs[1], outs[6]], [1, 6])
    lr_b = d4_ref.T(lr, 2)
    second = d4_ref.ensemble_mean([d4_ref.T_inv(inf.super_resolve(g, d4_ref.T(lr_b, k).to(dev)).cpu(), k) for k in (1, 6)], [1, 6])
    assert tuple(got3.shape) == (2,) + tuple(want.shape[1:])
    assert torch.equal(got3[0].cpu(), first[0]) and torch.equal(got3[1].cpu(), second[0])


@pytest.mark.parametrize("which", [0, 1])
def test_self_ensemble_batched_fp16_vs_oracle(dev, ensemble, which):
    """ensemble_batch=None (one call of 8 for the square input, two of 4 otherwise), fp16, against the CPU oracle's ensemble
    inverted and averaged in fp32: 0.02, the bound one fp16 forward is held to -- a mean of eight values each within it stays
    within it."""
    inf = P("infer")
    g, _, lrs, oracle = ensemble
    want = d4_ref.ensemble_mean(oracle[which], list(range(8)))
    got = inf.super_resolve(g, lrs[which].to(dev), self_ensemble=True, dtype=torch.float16).cpu()
    err = float((got - want).abs().max())
    print(f"self-ensemble fp16 batched vs oracle, LR {tuple(lrs[which].shape)}: max abs error {err:.3e}")
    assert err <= 0.02, err
    want2 = d4_ref.ensemble_mean([oracle[which][0], oracle[which][4]], [0, 4])
    got2 = inf.super_resolve(g, lrs[which].to(dev), self_ensemble=(0, 4)).cpu()
    assert float((got2 - want2).abs().max()) <= 0.02


def test_self_ensemble_tiled(dev, ensemble):
    inf = P("infer")
    g, _, lrs, _ = ensemble
    x = filler.tensor("in:d4_tiled", (1, 3, 40, 24), 0.5, 0.5).to(dev)
    whole = inf.super_resolve(g, x, self_ensemble=True)
    tiled = inf.super_resolve(g, x, tile=16, self_ensemble=True)
    assert tuple(whole.shape) == (1, 3, 160, 96)
    err = float((whole - tiled).abs().max())
    print(f"self-ensemble tiled vs whole: max abs difference {err:.3e}")
    assert err <= 2e-3, err


def test_evaluate_generator_self_ensemble(dev, ensemble):
    ev, inf = P("evaluate"), P("infer")
    g, _, lrs, _ = ensemble
    pairs = []
    for i, lr in enumerate(lrs):
        hr = filler.tensor(f"d4ev:hr{i}", (1, 3, 4 * lr.shape[2], 4 * lr.shape[3]), 0.5, 0.5)
        pairs.append((lr.to(dev), hr.to(dev), [f"img{i}"]))
    plain = ev.evaluate_generator(g, pairs)
    res = ev.evaluate_generator(g, pairs, self_ensemble=True)
    assert set(res) == set(plain) and list(res["psnr"]) == ["img0", "img1"] == list(res["ssim"])
    for lr, hr, name in pairs:
        sr = inf.super_resolve(g, lr, self_ensemble=True)
        assert res["psnr"][name[0]] == ev.psnr(sr, hr, None)
        # the same image scored in float64: only the fp32 reduction of the MSE differs (relative 1e-5 at most = 4e-5 dB)
        want = losses.psnr(sr.cpu(), hr.cpu(), max(float(hr.max()), 0.0) - min(float(hr.min()), 0.0))
        assert abs(res["psnr"][name[0]] - want) <= 1e-3
        assert res["psnr"][name[0]] != plain["psnr"][name[0]]
    assert res["avg_psnr"] == sum(res["psnr"].values()) / 2
