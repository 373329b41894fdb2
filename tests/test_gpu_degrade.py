"""GPU: the blind-degradation kernel (csrc/degrade.hip) and what is built on it -- utils.degradation.degrade_batch /
blur_downsample and PatchBank(degradation=...) -- against tests/degrade_ref.py (torch on the CPU in float64;
tests/test_host_degrade.py checks that yardstick itself).

With kernels whose weights are multiples of 2^-12 that sum to exactly 1, every product and every partial sum is a multiple
of 2^-12 not above 255 < 2^24 * 2^-12: fp32 holds them all, the result does not depend on rounding and is compared BIT FOR
BIT, scaling statements included.  Float kernels are held to a bound derived from the arithmetic (see the tests)."""
import importlib

import numpy as np
import pytest
import torch

import d4_ref
import degrade_ref

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
SIZES = [(37, 53), (64, 40), (150, 170)]                      # HR: partial tiles at every scale, several tiles at scale 8


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    P("_lib").lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def images(dev):
    rng = np.random.RandomState(31)
    host = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    return host, [torch.from_numpy(a).to(dev) for a in host]


_blur_cache = {}


def blur(host, n, kernel, s, offset):
    """the yardstick's float64 blur of image n, computed once per (image, kernel, scale, offset) and left unchanged"""
    key = (n, kernel.tobytes(), kernel.shape, s, offset)
    if key not in _blur_cache:
        _blur_cache[key] = degrade_ref.blur(host[n], kernel, s, offset)
    return _blur_cache[key]


def grid(shape, s, offset):
    return (shape[0] - offset + s - 1) // s, (shape[1] - offset + s - 1) // s


def corner_patches(h, w, ph, pw):
    """the four corners of an h x w LR grid and one patch inside"""
    return [(0, 0), (0, w - pw), (h - ph, 0), (h - ph, w - pw), ((h - ph) // 2, (w - pw) // 3)]


# ------------------------------------------------------------------ exact
@pytest.mark.parametrize("s", [1, 2, 3, 4, 8])
def test_exact_scales_sizes_offsets(dev, images, s):
    """Every (ks, offset, quantise) at this scale, on each image: five patches (the four corners of the LR grid and one inside)
    with two different kernels, whole-grid height or width where the grid is small."""
    D = P("utils.degradation")
    host, device = images
    _blur_cache.clear()
    for ks in (1, 3, 7, 21):
        kernels = [degrade_ref.dyadic_gaussian(ks, 0.5 + 0.11 * ks), degrade_ref.dyadic_gaussian(ks, 0.3 + 0.05 * ks)]
        for offset in sorted({0, s - 1}):
            for n in range(len(host)):
                h, w = grid(host[n].shape, s, offset)
                ph, pw = min(h, 19), min(w, 21)                # more than one 16 x 16 tile where the grid allows it
                pos = corner_patches(h, w, ph, pw)
                ks_b = np.stack([kernels[b % 2] for b in range(len(pos))])
                for quantise in (True, False):
                    got = D.degrade_batch([device[n]] * len(pos), [p[0] for p in pos], [p[1] for p in pos], ph, pw, s, ks_b,
                                          offset=offset, quantise=quantise).cpu()
                    for b, (t, l) in enumerate(pos):
                        ref = degrade_ref.finish(blur(host, n, kernels[b % 2], s, offset)[:, t:t + ph, l:l + pw], quantise=quantise)
                        want = degrade_ref.scale_f32(ref, degrade_ref.UNIT)
                        assert torch.equal(got[b], want), (ks, offset, n, quantise, b, float((got[b] - want).abs().max()))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_exact_modes_and_codes(dev, images, mode):
    """All eight codes on a square patch and the four shape-preserving ones on a non-square patch (both larger than a tile),
    in each scaling mode, quantised and not."""
    D = P("utils.degradation")
    host, device = images
    s, offset, ks = 2, 1, 7
    k = degrade_ref.dyadic_gaussian(ks, 1.2)
    h, w = grid(host[1].shape, s, offset)                      # 32 x 20
    for (ph, pw), codes in [((18, 18), list(range(8))), ((20, 17), [0, 2, 4, 6]), ((5, 19), [6, 4, 2, 0])]:
        n = len(codes)
        tops = [(3 * b) % (h - ph + 1) for b in range(n)]
        lefts = [(5 * b) % (w - pw + 1) for b in range(n)]
        tops[-1], lefts[-1] = h - ph, w - pw
        for quantise in (True, False):
            got = D.degrade_batch([device[1]] * n, tops, lefts, ph, pw, s, np.stack([k] * n), offset=offset, quantise=quantise,
                                  mode=mode, transforms=codes).cpu()
            for b in range(n):
                ref = degrade_ref.finish(blur(host, 1, k, s, offset)[:, tops[b]:tops[b] + ph, lefts[b]:lefts[b] + pw], quantise=quantise)
                want = d4_ref.T(degrade_ref.scale_f32(ref, mode), codes[b])
                assert torch.equal(got[b], want), ((ph, pw), codes[b], quantise)
    with pytest.raises(ValueError):
        D.degrade_batch([device[1]] * 2, [0, 0], [0, 0], 5, 19, s, np.stack([k] * 2), transforms=[1, 0])


def test_exact_seventy_samples(dev, images):
    """More than one chunk of the 64-entry table: 70 samples, images cycling, a different kernel, position and code each."""
    D = P("utils.degradation")
    host, device = images
    s, offset, ks, ph, pw = 3, 2, 7, 9, 9
    rng = np.random.RandomState(5)
    idx, tops, lefts, codes, ks_b = [], [], [], [], []
    for b in range(70):
        n = b % 3
        h, w = grid(host[n].shape, s, offset)
        idx.append(n), tops.append(int(rng.randint(0, h - ph + 1))), lefts.append(int(rng.randint(0, w - pw + 1)))
        codes.append(int(rng.randint(0, 8)))
        ks_b.append(degrade_ref.dyadic_gaussian(ks, 0.4 + 0.03 * b))
    got = D.degrade_batch([device[n] for n in idx], tops, lefts, ph, pw, s, np.stack(ks_b), offset=offset, mode=2, transforms=codes).cpu()
    assert tuple(got.shape) == (70, 3, ph, pw)
    for b in range(70):
        ref = degrade_ref.finish(blur(host, idx[b], ks_b[b], s, offset)[:, tops[b]:tops[b] + ph, lefts[b]:lefts[b] + pw])
        assert torch.equal(got[b], d4_ref.T(degrade_ref.scale_f32(ref, 2), codes[b])), b


# ------------------------------------------------------------------ float kernels, noise
def float_bound(ks):
    """ks^2 fused multiply-adds, each rounding a partial sum of at most 255 (the weights are non-negative and sum to 1): at most
    half an ulp of [128, 256) = 2^-17 each, ks^2 * 2^-17 in all, which over 255 is below ks^2 * 2^-24; plus the rounding of
    the division itself, and the weights' sum being 1 only to fp32: 2^-22."""
    return ks * ks * 2.0 ** -24 + 2.0 ** -22


@pytest.mark.parametrize("s,ks", [(4, 21), (8, 21), (1, 5), (3, 13)])
def test_float_kernels_within_the_derived_bound(dev, images, s, ks):
    D = P("utils.degradation")
    host, device = images
    kernels = D.random_kernels(5, ks, (0.2, 3.0), 0.5, np.random.RandomState(s * 100 + ks))
    worst = 0.0
    for n in range(len(host)):
        h, w = grid(host[n].shape, s, 0)
        ph, pw = min(h, 19), min(w, 21)
        pos = corner_patches(h, w, ph, pw)
        got = D.degrade_batch([device[n]] * 5, [p[0] for p in pos], [p[1] for p in pos], ph, pw, s, kernels, quantise=False).cpu()
        for b, (t, l) in enumerate(pos):
            ref = degrade_ref.finish(blur(host, n, kernels[b], s, 0)[:, t:t + ph, l:l + pw], quantise=False) / 255.0
            worst = max(worst, float((got[b].to(torch.float64) - ref).abs().max()))
    print(f"float kernels s={s} ks={ks}: max |got - ref| = {worst:.3e}, bound {float_bound(ks):.3e}")
    assert worst <= float_bound(ks)


def test_noise_levels_and_clipping(dev, images):
    """A given z and a noise level per sample: 0 (the result is then the noise-free one, bit for bit), moderate ones, and 200,
    which drives a good share of the pixels into both clips.  z is read at the OUTPUT position: checked with D4 codes."""
    D = P("utils.degradation")
    host, device = images
    s, ks, ph, pw = 2, 7, 18, 18
    stds = [0.0, 2.5, 25.0, 200.0, 7.0]
    codes = [0, 3, 5, 6, 1]
    kernels = D.random_kernels(5, ks, (0.2, 3.0), 0.5, np.random.RandomState(77))
    h, w = grid(host[0].shape, s, 0)
    pos = corner_patches(h, w, ph, pw)
    z = torch.from_numpy(np.random.RandomState(78).standard_normal((5, 3, ph, pw)).astype(np.float32))
    args = ([device[0]] * 5, [p[0] for p in pos], [p[1] for p in pos], ph, pw, s, kernels)
    got = D.degrade_batch(*args, noise=z.to(dev), noise_std=stds, quantise=False, transforms=codes).cpu()
    clean = D.degrade_batch(*args, quantise=False, transforms=codes).cpu()
    assert torch.equal(got[0], clean[0])
    # one more fused multiply-add; a result inside 0..255 is rounded by at most an ulp of a 0..255 value, 2^-16, which over 255
    # is the extra term (a result outside is clipped to the same end as the yardstick's: the two differ by far less than 1)
    bound = float_bound(ks) + 2.0 ** -16 / 255.0
    clipped = 0
    for b, (t, l) in enumerate(pos):
        acc = d4_ref.T(blur(host, 0, kernels[b], s, 0)[:, t:t + ph, l:l + pw], codes[b])
        ref = degrade_ref.finish(acc, z[b], stds[b], quantise=False) / 255.0
        err = float((got[b].to(torch.float64) - ref).abs().max())
        print(f"noise std={stds[b]}: max |got - ref| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (b, err)
        if stds[b] == 200.0:
            clipped = min(int((ref == 0.0).sum()), int((ref == 1.0).sum()))
        assert float(got[b].min()) >= 0.0 and float(got[b].max()) <= 1.0
    assert clipped > 50                                        # std 200 does clip, at both ends
    quant = D.degrade_batch(*args, noise=z.to(dev), noise_std=torch.tensor(stds).to(dev), quantise=True, transforms=codes).cpu() * 255.0
    assert torch.equal(quant, torch.round(quant)) and not torch.equal(quant, torch.round(clean * 255.0))
    with pytest.raises(ValueError):
        D.degrade_batch(*args, noise=z.to(dev))


# ------------------------------------------------------------------ patch = region of the whole image; determinism
@pytest.mark.parametrize("s,offset,ks", [(4, 0, 21), (8, 7, 21), (3, 1, 9), (1, 0, 3), (5, 2, 11)])
def test_patch_equals_the_region_of_the_whole_image(dev, images, s, offset, ks):
    """Float kernels: the tap order does not depend on the tile or the patch position, so the bits agree.  The whole image is
    also the yardstick's to within one grey level, and equal to it wherever the yardstick is not near a rounding tie."""
    D = P("utils.degradation")
    host, device = images
    k = D.random_kernels(1, ks, (0.6, 2.5), 0.0, np.random.RandomState(9))[0]
    for n in range(len(host)):
        whole = D.blur_downsample(device[n], k, s, offset)
        h, w = grid(host[n].shape, s, offset)
        assert whole.dtype == torch.uint8 and tuple(whole.shape) == (h, w, 3)
        planar = whole.permute(2, 0, 1).to(torch.float32).cpu()
        ref = degrade_ref.finish(blur(host, n, k, s, offset), quantise=False)
        sure = (ref - torch.round(ref)).abs() < 0.49
        assert torch.equal(planar.to(torch.float64)[sure], torch.round(ref)[sure]) and float((planar - ref).abs().max()) <= 0.51
        ph, pw = min(h, 17), min(w, 13)
        pos = corner_patches(h, w, ph, pw) + [(min(1, h - ph), min(2, w - pw))]
        got = D.degrade_batch([device[n]] * len(pos), [p[0] for p in pos], [p[1] for p in pos], ph, pw, s, np.stack([k] * len(pos)),
                              offset=offset, quantise=True).cpu() * 255.0
        for b, (t, l) in enumerate(pos):
            assert torch.equal(got[b], planar[:, t:t + ph, l:l + pw]), (n, b)
    # numpy in, numpy out; noise from a seeded generator is reproducible and does something
    arr = D.blur_downsample(host[0], k, s, offset)
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, D.blur_downsample(device[0], k, s, offset).cpu().numpy())
    g = torch.Generator(device=dev)
    noisy = [D.blur_downsample(device[0], k, s, offset, noise_std=10.0, generator=g.manual_seed(4)) for _ in range(2)]
    assert torch.equal(noisy[0], noisy[1]) and not torch.equal(noisy[0].cpu(), torch.from_numpy(arr))


def test_two_runs_give_the_same_bits(dev, images):
    D = P("utils.degradation")
    host, device = images
    kernels = D.random_kernels(6, 21, (0.2, 3.0), 0.5, np.random.RandomState(1))
    z = torch.randn((6, 3, 30, 30), device=dev)
    std = torch.tensor([0.0, 1.0, 5.0, 10.0, 25.0, 50.0], device=dev)
    run = lambda: D.degrade_batch([device[2]] * 6, [0, 1, 2, 3, 4, 7], [12, 0, 5, 3, 1, 9], 30, 30, 4, kernels, noise=z, noise_std=std,
                                  quantise=False, transforms=[0, 1, 2, 3, 4, 5])
    a, b = run(), run()
    assert torch.equal(a, b)


# ------------------------------------------------------------------ PatchBank
class RecordingRng:
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.calls = []

    def randint(self, *a):
        v = self.rs.randint(*a)
        self.calls.append(("randint", a, v))
        return v

    def uniform(self, *a):
        v = self.rs.uniform(*a)
        self.calls.append(("uniform", a, v))
        return v


@pytest.fixture(scope="module")
def bank_pairs(dev):
    rng = np.random.RandomState(29)
    u8 = lambda h, w: torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)
    return [(u8(24, 40), u8(96, 160)), (None, u8(115, 131)), (u8(32, 56), u8(128, 224))]


@pytest.mark.parametrize("patch", [(16, 16), (16, 8)])
def test_patch_bank_with_a_degradation(dev, bank_pairs, patch):
    """The LR batch is the yardstick applied with bank.last_kernels at the positions and codes that the recording rng saw
    (float kernels, not quantised: the bound of the float-kernel test); the HR batch is that of the same bank without it."""
    DS = P("dataset")
    pw, ph = patch
    batch, seed, s = 12, 41, 4
    rec = RecordingRng(seed)
    bank = DS.PatchBank(bank_pairs, s, patch, rng=rec, augment=True, reference_scaling=False,
                        degradation=DS.BlindDegradation(kernel_size=9, offset=1, quantise=False))
    lr, hr = bank.sample(batch)
    assert tuple(lr.shape) == (batch, 3, ph, pw) and tuple(hr.shape) == (batch, 3, s * ph, s * pw)
    assert len(rec.calls) == 4 * batch + 4 * batch                     # indices, (x, y) each, codes; four uniforms per kernel
    draws = [int(c[2]) for c in rec.calls[:4 * batch]]
    idx, codes = draws[:batch], draws[3 * batch:4 * batch]
    if pw != ph:
        codes = [2 * k for k in codes]
    kernels = bank.last_kernels.cpu().numpy()
    assert bank.last_kernels.is_cuda and kernels.shape == (batch, 9, 9) and bank.last_noise_std is None
    refs = []
    for b in range(batch):
        cx, cy = draws[batch + 2 * b], draws[batch + 2 * b + 1]
        top, left = cy - ph // 2, cx - pw // 2
        acc = degrade_ref.blur(bank_pairs[idx[b]][1].cpu(), kernels[b], s, 1)[:, top:top + ph, left:left + pw]
        refs.append(d4_ref.T(degrade_ref.finish(acc, quantise=False), codes[b]))
        err = float((lr[b].cpu().to(torch.float64) - refs[b] / 255.0).abs().max())
        assert err <= float_bound(9), (b, err)
    # the same bank, quantising: whole grey levels, the yardstick's wherever that is not at a rounding tie
    quant = DS.PatchBank(bank_pairs, s, patch, rng=np.random.RandomState(seed), augment=True, reference_scaling=False,
                         degradation=DS.BlindDegradation(kernel_size=9, offset=1))
    grey = quant.sample(batch)[0].cpu() * 255.0
    assert torch.equal(quant.last_kernels, bank.last_kernels)
    for b in range(batch):
        sure = (refs[b] - torch.round(refs[b])).abs() < 0.49
        assert torch.equal(grey[b].to(torch.float64)[sure], torch.round(refs[b])[sure]), b
        assert float((grey[b] - refs[b]).abs().max()) <= 0.51
    # the HR batch: bit-equal to what the same seeded bank returns without the degradation (pair 1 needs an LR image there)
    full = [(p[0] if p[0] is not None else torch.zeros((28, 32, 3), dtype=torch.uint8, device=dev), p[1]) for p in bank_pairs]
    lr0, hr0 = DS.PatchBank(full, s, patch, rng=np.random.RandomState(seed), augment=True, reference_scaling=False).sample(batch)
    assert torch.equal(hr, hr0)
    # explicit kernels: a delta kernel at offset 0 is plain decimation of the HR patch (HR is u / 255 * 2 - 1: undone to 2^-23)
    delta = np.zeros((batch, 3, 3), dtype=np.float32)
    delta[:, 1, 1] = 1.0
    unit = DS.PatchBank(bank_pairs, s, patch, rng=np.random.RandomState(seed), reference_scaling=False,
                        degradation=DS.BlindDegradation(kernel_size=3))
    lr1, hr1 = unit.sample(batch, kernels=delta)
    assert float((lr1 - ((hr1 + 1.0) / 2.0)[:, :, ::s, ::s]).abs().max()) <= 2.0 ** -23
    # noise levels drawn per sample, z from a seeded device generator: reproducible
    g = torch.Generator(device=dev)
    outs = []
    for _ in range(2):
        noisy = DS.PatchBank(bank_pairs, s, patch, rng=np.random.RandomState(seed),
                             degradation=DS.BlindDegradation(kernel_size=5, noise_std=(2.0, 20.0)), generator=g.manual_seed(3))
        outs.append(noisy.sample(batch)[0])
        assert tuple(noisy.last_noise_std.shape) == (batch,) and float(noisy.last_noise_std.min()) >= 2.0
    assert torch.equal(outs[0], outs[1])


def test_patch_bank_without_degradation_is_unchanged(dev, bank_pairs):
    """degradation=None: the draws and the bits of the two patch_batch launches, called directly here."""
    DS = P("dataset")
    pairs = [bank_pairs[0], bank_pairs[2]]
    patch, batch, seed = (16, 8), 9, 13
    rng = np.random.RandomState(seed)
    idx = [int(rng.randint(0, 2)) for _ in range(batch)]
    coords = [DS.train_patch_coords(pairs[i][0].shape[0], pairs[i][0].shape[1], patch, 4, rng) for i in idx]
    codes = [2 * int(rng.randint(0, 4)) for _ in range(batch)]
    want_lr = DS.patch_batch([pairs[i][0] for i in idx], [c[0] for c in coords], [c[1] for c in coords], 8, 16, DS.PATCH_LR_REF, codes)
    want_hr = DS.patch_batch([pairs[i][1] for i in idx], [c[2] for c in coords], [c[3] for c in coords], 32, 64, DS.PATCH_HR_REF, codes)
    used = np.random.RandomState(seed)
    bank = DS.PatchBank(pairs, 4, patch, rng=used, augment=True)
    lr, hr = bank.sample(batch)
    assert torch.equal(lr, want_lr) and torch.equal(hr, want_hr) and bank.last_kernels is None
    assert used.randint(0, 1 << 30) == rng.randint(0, 1 << 30)                               # and nothing drawn beyond them


# ------------------------------------------------------------------ graph replay
def test_graph_replay_follows_the_kernel_tensor(dev, images):
    """Captured with preallocated inputs, the launch reads the kernels (and the noise) when it is replayed."""
    D = P("utils.degradation")
    host, device = images
    s, ks, ph, pw, n = 4, 21, 20, 24, 3
    k_host = [D.random_kernels(n, ks, (0.2, 3.0), 0.5, np.random.RandomState(seed)) for seed in (1, 2)]
    k_dev = torch.from_numpy(k_host[0]).to(dev)
    z = torch.zeros((n, 3, ph, pw), device=dev)
    std = torch.tensor([0.0, 4.0, 9.0], device=dev)
    args = ([device[2]] * n, [0, 5, 17], [18, 0, 7], ph, pw, s)
    eager = [D.degrade_batch(*args, torch.from_numpy(k).to(dev), noise=z, noise_std=std, transforms=[0, 2, 6]).clone() for k in k_host]
    assert not torch.equal(eager[0], eager[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.degrade_batch(*args, k_dev, noise=z, noise_std=std, transforms=[0, 2, 6])          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = D.degrade_batch(*args, k_dev, noise=z, noise_std=std, transforms=[0, 2, 6])
    graph.replay()
    assert torch.equal(out, eager[0])
    k_dev.copy_(torch.from_numpy(k_host[1]).to(dev))
    graph.replay()
    assert torch.equal(out, eager[1])
    z.copy_(torch.randn(z.shape, device=dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[1][0]) and not torch.equal(out[1], eager[1][1])         # std 0 / std 4
