"""CPU: the case tables, references and bounds of the style-kernel sweep (tests/style_sweep_ref.py), checked without a device.

1. every case is on the far side of the threshold it is there for, by the restated launcher arithmetic and by what the ABI
   reports, and the counts the tables rest on are pinned;
2. every branch that a production tap takes (the five taps of Real-ESRGAN's feature loss at crops of 128 and 256, batches of 4
   and 16) is taken by a sweep case of the kernel it concerns;
3. an fp32 evaluation of the correct formulas, chunked like the kernels, lies inside the float bands;
4. every listed wrong variant fails the exact comparison of at least one case, and the test names the case;
5. what torch does in float64 with a NaN or an Inf in a Gram matrix, next to what the kernels do on purpose."""
import importlib
import math

import pytest
import torch

import style_sweep_ref as R

PKG = "deep-super-resolution_amd"
DT = [pytest.param(v, id=k) for k, v in R.DTYPES.items()]


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + "._lib").lib()


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_references():
    yield
    R.drop_caches()


# ============================================================================= 1. thresholds
def test_constants_are_the_ones_the_package_and_the_first_regime_tests_use():
    L = importlib.import_module(PKG + "._lib")
    assert L.GRAM_LOSS_PARTIALS == R.GRAM_LOSS_PARTIALS == 2 * R.DSR_GRAM_LOSS_SLICES == 64
    assert R.GRAM_CHUNK % R.GRAM_KP == 0 and R.STYLE_MAX_CP == 8 * R.TILE
    for dtype in R.DTYPES.values():                       # the margins keep every buffer 16-byte aligned
        assert (R.MARGIN * torch.empty(0, dtype=dtype).element_size()) % 16 == 0
    assert R.MARGIN * 4 % 16 == 0 and R.MARGIN * 8 % 16 == 0


def test_gram_forward_cases_are_past_their_thresholds(lib):
    reg = {k: R.regime(*v) for k, v in R.FWD_CASES.items()}
    for name, (n, hw, c, cp) in R.FWD_CASES.items():
        assert 1 <= c <= cp <= R.STYLE_MAX_CP and cp % 8 == 0 and 9 * hw < 2 ** 24, name
        assert lib.dsr_gram_chunks(hw) == R.chunks(hw), name
        assert lib.dsr_gram_workspace(n, hw, cp) == n * R.chunks(hw) * cp * cp, name
    # cp72: two tiles, the second 8 channels wide; 200 pixels = one whole staging step and a ragged one of 72
    assert reg["cp72"].tiles == 2 and 72 - 64 == 8 and reg["cp72"].last_tile_partial
    assert 200 // R.GRAM_KP == 1 and 200 % R.GRAM_KP == 72 and reg["cp72"].last_chunk == "ragged"
    # cp200-pad: four tiles, ten pairs, the last tile 8 channels wide, pad channels, gram's row stride odd
    assert (R.tiles(200), R.pairs(200)) == (4, 10) and 200 - 3 * 64 == 8 and reg["cp200-pad"].pad and 197 % 2 == 1
    # cp512-edge: 36 pairs, two chunks, the second one pixel
    assert (R.tiles(512), R.pairs(512)) == (8, 36) and R.chunks(1025) == 2 and reg["cp512-edge"].last_chunk == "one"
    # hw1024 / hw2048: px1 = HW through the other arm of the ternary, one and two chunks
    assert R.chunks(1024) == 1 and R.chunks(2048) == 2 and 1024 == R.GRAM_CHUNK
    assert reg["hw1024"].last_chunk == reg["hw2048"].last_chunk == "full"
    assert not reg["hw1024"].multi_chunk and reg["hw2048"].multi_chunk
    # chunks9: nine chunks in each of three images, the last one pixel
    assert R.chunks(8193) == 9 and 8193 - 8 * 1024 == 1 and R.FWD_CASES["chunks9"][0] == 3 and reg["chunks9"].last_chunk == "one"
    # foldcap: the only case past the fold's grid, with a ragged second pass
    assert R.fold_items(5, 459) == 1053405 and R.GRAM_FOLD_CAP == 1048576
    assert R.GRAM_FOLD_CAP < 1053405 < 2 * R.GRAM_FOLD_CAP
    assert [k for k, r in reg.items() if r.fold_past_cap] == ["foldcap"]
    assert 464 - 7 * 64 == 16 and reg["foldcap"].pad and reg["foldcap"].tiles == 8
    assert R.fold_items(4, 512) == R.GRAM_FOLD_CAP and R.fold_items(16, 256) == R.GRAM_FOLD_CAP       # N = 5 and 17 are the first past
    # the split that C = 459 takes in the loss (the case is a forward case; the count is what its name rests on)
    assert (R.slices(459), R.per(459), 459 * 459 - 25 * R.per(459)) == (26, 8104, 8081)
    for name in R.FWD_CASES:                              # exact in fp32 whatever the order, and not vacuous
        slabs, gram = R.fwd_reference(name)
        n, hw, c, cp = R.FWD_CASES[name]
        assert float(slabs.abs().max()) < 2 ** 24 and float(gram.abs().max()) < 2 ** 24
        assert bool((slabs[:, -1, 0, 0] >= 9).all())      # the last chunk of every image counts, a one-pixel chunk too
        assert not bool(slabs[:, :, c:, :].any()) and bool((gram != 0).any())


def _largest(t):
    return int(t.max()) if t.numel() else 0


def test_gram_loss_cases_are_past_their_thresholds():
    want = {"c90-1slice": (1, False), "c91-2slices-ragged": (2, True), "c128-2slices": (2, False), "c200-5slices": (5, False),
            "c256-8slices": (8, False), "c512-32slices": (32, False), "n129-258terms": (2, True), "n9-288terms": (32, False)}
    for name, (n, c, cp) in R.LOSS_CASES.items():
        r = R.regime(n, 1, c, cp)
        assert (r.slices, r.last_slice_ragged) == want[name], name
        assert 2 * R.loss_terms(n, c) <= R.GRAM_LOSS_PARTIALS * n and n <= 65535
        gf, gt = R.loss_input(name)
        assert int(gf.abs().max()) <= 20 and int(gt.abs().max()) <= 20
        d = gf - gt
        mx = d.abs().reshape(n, -1).amax(1)
        sums, maxs = R.loss_partials(d, 1)
        assert int(mx[0]) == int(mx[n - 1]) == R.PLANT == 37 and _largest(d.abs().reshape(n, -1)[1:n - 1]) <= 36
        assert int((d.abs() == R.PLANT).sum()) == 2
        assert int(maxs[0, -1]) == 37 and _largest(maxs[0, :-1]) <= 36                    # only image 0's LAST slice holds its maximum
        assert int(maxs[n - 1, 0]) == 37 and _largest(maxs[n - 1, 1:]) <= 36              # only the last image's slice 0 holds its own
        assert int(d[0].reshape(-1)[-1]) == 37 and int(d[n - 1].reshape(-1)[0]) == -37
        assert bool((d[0] == 0).any()) and bool((d[0] > 0).any()) and bool((d[0] < 0).any())      # sign(d) takes its three values
        if n >= 3:
            assert not bool(d[1].any()) and bool((sums[1] == 0).all())
        assert int(sums.sum()) < 2 ** 53
    assert R.per(91) == 4141 and 91 * 91 - R.per(91) == 4140                              # the ragged second slice
    assert R.slices(90) == 1 and R.slices(91) == 2                                        # 90 is the last C with one slice
    assert (R.loss_terms(129, 91), R.loss_terms(9, 512)) == (258, 288)
    assert [k for k, v in R.LOSS_CASES.items() if R.regime(v[0], 1, v[1], v[2]).terms_past_256] == ["n129-258terms", "n9-288terms"]
    assert [R.slices(c) for c in (64, 128, 256, 512)] == [1, 2, 8, 32]
    n, c, cp = R.NONFINITE_SHAPE
    assert R.slices(c) == 8 and n == 3


def test_tap_backward_cases_are_past_their_thresholds():
    reg = {k: R.regime(*v) for k, v in R.BWD_CASES.items()}
    assert [r.ksteps for r in reg.values()] == [1, 2, 4, 8]
    assert [r.last_kstep_ragged for r in reg.values()] == [False, True, True, False]
    assert [r.last_pixel_tile_ragged for r in reg.values()] == [False, True, True, True]
    assert [r.pad for r in reg.values()] == [False, False, True, False]
    assert R.pixel_tiles(64) == 1 and R.pixel_tiles(65) == 2 and R.pixel_tiles(130) == 3 and R.pixel_tiles(70) == 2
    assert R.BWD_CASES["hw64"][0] == 3                   # blockIdx.x = n * tilesP + tile with one tile per image
    for name, (n, hw, c, cp) in R.BWD_CASES.items():
        assert 6 * cp <= 3072
        flags = R.bwd_flags(name)
        assert len(flags) == (12 if name in R.BWD_ALL_FLAGS else 3) and len(set(flags)) == len(flags)
        assert {f[0] for f in flags if f[3]} == {0, 1}
    # the one rounding does round somewhere, in both formats, in every case
    for name in R.BWD_CASES:
        for dtype in R.DTYPES.values():
            inexact = 0
            for flags in R.bwd_flags(name):
                want = R.bwd_expected(name, *flags)
                inexact += int((want.float().to(dtype).double() != want).sum())
            assert inexact > 0, (name, dtype)


# ============================================================================= 2. coverage of the production shapes
FIVE_C = (64, 128, 256, 512, 512)        # conv1_2, conv2_2, conv3_4, conv4_4, conv5_4 (FIVE in tests/test_gpu_vggstyle.py)


def _production_regimes():
    out = []
    for s in (128, 256):
        for n in (4, 16):
            for k, c in enumerate(FIVE_C):
                out.append(((n, s * s // 4 ** k, c, c), R.regime(n, s * s // 4 ** k, c, c)))
    return out


def test_every_branch_of_a_production_tap_is_taken_by_a_sweep_case():
    """A later change of a cap (the fold's grid, the slice size, the chunk) moves production shapes or sweep cases across a
    threshold: then a component value of a production regime has no case any more, and this test says which."""
    cases = {"fwd": [R.regime(*v) for v in R.FWD_CASES.values()],
             "loss": [R.regime(n, 1, c, cp) for n, c, cp in R.LOSS_CASES.values()],
             "bwd": [R.regime(*v) for v in R.BWD_CASES.values()]}
    prod = _production_regimes()
    assert len(prod) == 20 and {p[0][1] for p in prod} == {65536, 16384, 4096, 1024, 256, 64}
    missing = []
    for kernel, fields in R.REGIME_FIELDS.items():
        for field in fields:
            have = {getattr(r, field) for r in cases[kernel]}
            for shape, r in prod:
                if getattr(r, field) not in have:
                    missing.append((kernel, field, getattr(r, field), shape))
    assert not missing, missing
    # what production does reach, so that the assertion above is seen to bite
    seen = {f: {getattr(r, f) for _, r in prod} for f in R.Regime._fields}
    assert seen["tiles"] == {1, 2, 4, 8} and seen["slices"] == {1, 2, 8, 32} and seen["ksteps"] == {1, 2, 4, 8}
    assert seen["fold_past_cap"] == {False, True} and seen["terms_past_256"] == {False, True}
    assert seen["multi_chunk"] == {False, True} and seen["last_chunk"] == {"full", "ragged"}
    # and the sweep goes where production does not: the partial tile, pad channels, the one-pixel chunk, the ragged slice
    assert any(r.last_tile_partial for r in cases["fwd"]) and any(r.pad for r in cases["fwd"])
    assert any(r.last_chunk == "one" for r in cases["fwd"]) and any(r.last_slice_ragged for r in cases["loss"])
    assert any(r.last_kstep_ragged for r in cases["bwd"]) and any(r.last_pixel_tile_ragged for r in cases["bwd"])


# ============================================================================= 3. fp32 inside the float bands
_FP32_RATIOS = {}


@pytest.mark.parametrize("name", list(R.FLOAT_CASES))
@pytest.mark.parametrize("dtype", DT)
def test_fp32_evaluation_is_inside_the_float_bands(dtype, name):
    """Forward: per-chunk fp32 products (torch's fp32 matmul), the chunks added in order in fp32, one fp32 product with the
    scale.  Loss: double sums, one rounding.  Backward: the 16-bit operand as the kernel forms it, an fp32 GEMM, the fp32
    epilogue, one rounding."""
    n, hw, c, cp = R.FLOAT_CASES[name]
    scale = R.float_scale(name)
    grams = []
    for which in (0, 1):
        ref, bound = R.float_fwd_reference(name, dtype, which)
        x = R.float_input(name, dtype)[which]
        got = R.fold_slabs(R.chunk_products(x, torch.float32), c, scale, torch.float32)
        assert got.dtype == torch.float32
        ratio = R.worst_ratio((got.double() - ref).abs(), bound)
        print(f"style sweep fp32 emulation {name} {dtype}: forward max err/bound = {ratio:.3f}")
        assert ratio <= 1.0
        grams.append(got)
    d64 = grams[0].double() - grams[1].double()
    for mode in (0, 1):
        value, s16, ss = R.emulate_loss_operand(d64, mode, dtype)
        v64 = R.float_loss_reference(d64, mode)
        assert abs(float(value) - v64) <= 2.0 ** -23 * v64
        coef, g_up, ref, bound = R.float_bwd_reference(name, dtype, d64, mode)
        assert 3.0 <= float(ref.abs().max()) < 6.0
        df = R.emulate_bwd_style_only(R.float_input(name, dtype)[0], s16, ss, g_up, coef, c)
        ratio = R.worst_ratio((df.double() - ref).abs(), bound)
        print(f"style sweep fp32 emulation {name} {dtype} mode {mode}: backward max err/bound = {ratio:.3f}")
        assert ratio <= 1.0
        assert not bool(df[..., c:].any())


# ============================================================================= 4. wrong variants fail
def _fwd_failures(variant):
    out = []
    for name, (n, hw, c, cp) in R.FWD_CASES.items():
        slabs, gram = R.fwd_reference(name)
        for scale in R.FWD_SCALES:
            if not torch.equal(R.fold_slabs(slabs, c, scale, variant=variant), gram * scale) and name not in out:
                out.append(name)
    return out


def _loss_failures(variant):
    out = []
    for name, (n, c, cp) in R.LOSS_CASES.items():
        gf, gt = R.loss_input(name)
        d = gf - gt
        for mode in (0, 1):
            v, ss = R.loss_expected(d, mode)
            bv, bss = R.loss_expected(d, mode, variant)
            if (v != bv or not torch.equal(ss, bss)) and name not in out:
                out.append(name)
    return out


def _bwd_failures(variant):
    out = []
    for name in R.BWD_CASES:
        for dtype in R.DTYPES.values():
            for flags in R.bwd_flags(name):
                good = R.bwd_expected(name, *flags).float().to(dtype)
                bad = R.bwd_expected(name, *flags, variant=variant).float().to(dtype)
                if not torch.equal(good, bad) and name not in out:
                    out.append(name)
    return out


MULTI_SLICE = [k for k, (n, c, cp) in R.LOSS_CASES.items() if R.slices(c) > 1]
WRONG = {
    # variant: (which comparison, exactly the cases that reject it)
    "one-grid-pass": (_fwd_failures, ["foldcap"]),                           # only the case past the cap sees the second pass
    "chunks-1": (_fwd_failures, list(R.FWD_CASES)),                          # the one-pixel last chunks included
    "row-stride-cp": (_fwd_failures, ["cp200-pad", "chunks9", "foldcap"]),   # the cases with C < Cp
    "no-last-slice": (_loss_failures, list(R.LOSS_CASES)),                   # (with one slice the last slice is everything)
    "max-slice-0": (_loss_failures, MULTI_SLICE),
    "terms-256": (_loss_failures, ["n129-258terms", "n9-288terms"]),
    "k448": (_bwd_failures, ["cp512"]),                                      # the only case with K > 448
    "s16-transposed": (_bwd_failures, list(R.BWD_CASES)),
}


@pytest.mark.parametrize("variant", list(WRONG))
def test_wrong_variant_fails_the_named_cases(variant):
    assert set(WRONG) == set(R.FWD_VARIANTS + R.LOSS_VARIANTS + R.BWD_VARIANTS)
    failures, named = WRONG[variant]
    caught = failures(variant)
    print(f"{variant}: rejected by {caught}")
    assert caught and set(caught) == set(named)
    assert failures(None) == []                           # the correct formula fails none


def test_a_dropped_slice_moves_the_value_far_past_one_ulp():
    """What the 3e-2 bar of the module test cannot see: one slice of 32 is about 3 % of the value, thousands of fp32 ulps."""
    gf, gt = R.loss_input("c512-32slices")
    d = gf - gt
    for mode in (0, 1):
        good, bad = float(R.loss_expected(d, mode)[0]), float(R.loss_expected(d, mode, "no-last-slice")[0])
        rel = (good - bad) / good
        assert 0.02 < rel < 0.04 and rel > 1000 * 2.0 ** -23


# ============================================================================= 5. non-finite entries
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_torch_policy_for_a_non_finite_gram_entry(bad):
    """torch, float64: the value is not finite in both modes.  mse_loss hands the NaN or the Inf on to the gradient.  l1_loss does
    not: its gradient is sign(d) / count, which is 0 at a NaN and 1 / count at +Inf, so F . dG is finite everywhere and a loss
    scaler that reads gradients would never see the overflow.  The kernels differ from that on purpose: dsr_gram_loss stores a
    non-finite difference in s16 as it is, in both modes (and a non-finite maximum in s_scale for MSE), so that
    dsr_featstyle_tap_bwd writes non-finite values into df of that image -- and of that image alone
    (tests/test_gpu_style_sweep.py)."""
    n, c, _ = R.NONFINITE_SHAPE
    img, i, j = R.NONFINITE_AT
    gf, gt, f = R.nonfinite_input()
    assert not bool((f == 0).any()) and bool(((gf - gt)[1] != 0).any())
    for mode in (0, 1):
        value, dg, fdg = R.torch_nonfinite_gram(mode, bad)
        assert not math.isfinite(float(value))
        assert math.isnan(float(value)) == math.isnan(bad)
        others = torch.ones(n, c, c, dtype=torch.bool)
        others[img, i, j] = False
        assert bool(torch.isfinite(dg[others]).all())
        if mode == 0:
            assert float(dg[img, i, j]) == (0.0 if math.isnan(bad) else 1.0 / (n * c * c))
            assert bool(torch.isfinite(fdg).all())
        else:
            assert not math.isfinite(float(dg[img, i, j])) and math.isnan(float(dg[img, i, j])) == math.isnan(bad)
            assert not bool(torch.isfinite(fdg[img, :, j]).any()) and bool(torch.isfinite(fdg[[0, 2]]).all())


def test_guard_sees_a_write_outside_and_poisons_a_read_outside():
    g = R.Guard(torch.device("cpu"))
    out = g.new((3, 5), torch.float32)
    x = g.put(torch.ones(7, dtype=torch.bfloat16))
    assert bool((out == R.SENTINEL).all()) and out.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    g.check()
    flat = g.bufs[1][0]
    assert bool(torch.isnan(flat[:R.MARGIN]).all()) and bool(torch.isnan(flat[-R.MARGIN:]).all())       # an input's margins
    g.bufs[0][0][R.MARGIN + 15] = 1.0                                                              # one element past the end
    with pytest.raises(AssertionError, match="outside"):
        g.check()
