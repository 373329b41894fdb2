"""CPU: what tests/test_gpu_luma_sweep.py relies on, without a device -- each case of tests/luma_sweep_ref.py has the block count
listed (dsr_luma_blocks of the built library); an fp32 emulation of luma_kernel in its own order (stride-256 fused accumulation,
xor butterfly, (r0 + r1) + (r2 + r3)) is inside the per-block bound on every case, in both `quantize` modes and in all nine dtype
pairs on `ragged`; three wrong variants are outside it; the positions, the closed form and the synthetic table of the other
tests are what they say."""
import importlib
import math

import pytest
import torch

import luma_ref
import luma_sweep_ref as R

PKG = "deep-super-resolution_amd"
PAIRS = [(a, b) for a in R.DTYPES for b in R.DTYPES]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def lib():
    P("_build").build()
    return P("_lib").lib()


def test_each_case_has_the_block_count_listed(lib):
    for name, (n, H, W, s, B) in R.CASES.items():
        h, w = R.region(name)
        assert lib.dsr_luma_blocks(n, H, W, s) == n * B, name
        assert R.blocks_of(h * w) == B, name
    assert [R.region(k)[0] * R.region(k)[1] for k in R.CASES] == [7360, 4096, 4097, 8192, 7360, 267273]
    assert 7360 - 4096 == 3264 and 4096 % 115 != 0                     # ragged: a row straddles the block edge
    assert R.CASES["many"][0] > 16 and R.CASES["long"][4] > 64 and max(v[4] for k, v in R.CASES.items() if k != "long") < 64
    n, H, W, s, B = R.FIN
    assert lib.dsr_luma_blocks(n, H, W, s) == n * B and n > 32 and B > 128
    # the shapes of tests/test_gpu_luma.py never leave one block per image
    for hw in ((23, 37), (32, 32), (48, 64)):
        assert lib.dsr_luma_blocks(1, hw[0], hw[1], 0) == 1


@pytest.mark.parametrize("quantize", [False, True], ids=["values", "quantize"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_emulation_is_inside_the_bound(name, quantize):
    p, t = R.inputs(name)
    s = R.CASES[name][3]
    want, bound = R.reference(name, quantize)
    assert want.shape == (R.CASES[name][0] * R.CASES[name][4],) and bool((bound > 0).all())
    d = R.emulate_dy(p, t, s, quantize)
    ratio = R.worst_ratio(R.emulate_blocks(d), want, bound)
    print(f"{name} quantize={quantize}: fp32 emulation, largest |emulation - f64| / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("quantize", [False, True], ids=["values", "quantize"])
@pytest.mark.parametrize("dp,dt", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_emulation_is_inside_the_bound_in_every_dtype_pair(dp, dt, quantize):
    p, t = R.inputs("ragged", dp, dt)
    want, bound = R.reference("ragged", quantize, dp, dt)
    ratio = R.worst_ratio(R.emulate_blocks(R.emulate_dy(p, t, 3, quantize)), want, bound)
    print(f"ragged {dp} / {dt} quantize={quantize}: largest |emulation - f64| / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_sequential_sum_shows_how_tight_the_bound_is():
    """One fp32 accumulator running over a 4096-pixel chunk is tens of u off, relative (about 50 u on `long`, which is about
    the bound itself: 24 u for the sum plus 2 c u for dY), while the kernel's order -- 16 terms per thread, then a tree -- stays
    within a twentieth of it (above).  The figure is printed; only its order of magnitude is asserted."""
    p, t = R.inputs("long")
    want, bound = R.reference("long", True)
    seq = R.sequential_blocks(R.emulate_dy(p, t, 1, True))
    rel = ((seq.double() - want).abs() / want).max().item() / R.U
    ratio = R.worst_ratio(seq, want, bound)
    print(f"long: sequential fp32 sum, largest relative error {rel:.1f} u, {ratio:.3f} of the bound")
    assert rel > 10.0


@pytest.mark.parametrize("quantize", [False, True], ids=["values", "quantize"])
@pytest.mark.parametrize("name", ["ragged", "plus-one", "two-full", "many", "long"])
def test_neighbouring_chunk_is_outside_the_bound(name, quantize):
    """partial[j] holding chunk j + 1 (or j - 1): an off-by-one in blk, or n / B and n % B confused."""
    p, t = R.inputs(name)
    want, bound = R.reference(name, quantize)
    emu = R.emulate_blocks(R.emulate_dy(p, t, R.CASES[name][3], quantize)).double()
    for shift in (1, -1):
        err = (torch.roll(emu, shift) - want).abs()
        assert bool((err > bound).all()), (name, shift)


@pytest.mark.parametrize("quantize", [False, True], ids=["values", "quantize"])
@pytest.mark.parametrize("name", ["ragged", "many", "long"])
def test_unguarded_last_block_is_outside_the_bound(name, quantize):
    """A last block without `i < hw` sums on into the next image."""
    p, t = R.inputs(name)
    n, _, _, s, B = R.CASES[name]
    want, bound = R.reference(name, quantize)
    emu = R.emulate_blocks(R.emulate_dy(p, t, s, quantize), guard=False).double()
    err = ((emu - want).abs() / bound).view(n, B)
    assert bool((err[:-1, -1] > 1.0).all())                            # the last block of every image that has a next one
    assert bool((err[:, :-1] <= 1.0).all()) and bool(err[-1, -1] <= 1.0)


def test_subtracted_lumas_are_outside_the_bound_on_near_identical_images():
    """preds = target except four green codes per chunk one step up: dY = 128.553 / 255^2 = 2e-3 at those pixels, while two
    lumas of ~0.4 carry ~3e-8 of rounding each.  The channel differences taken first are exact there."""
    n, H, W, s, B = R.CASES["ragged"]
    h, w = R.region("ragged")
    g = torch.Generator().manual_seed(9)
    t = torch.randint(0, 255, (n, 3, H, W), generator=g).float() / 255.0
    p = t.clone()
    for i in range(0, h * w, 1024):
        p[:, 1, i // w + s, i % w + s] += 1.0 / 255.0
    want, bound = R.table_and_bound(p, t, s, True)
    assert abs(want[0].item() - 4 * (128.553 / 255.0 ** 2) ** 2) <= 1e-15
    good = R.worst_ratio(R.emulate_blocks(R.emulate_dy(p, t, s, True)), want, bound)
    bad = (R.emulate_blocks(R.emulate_dy(p, t, s, True, subtract_lumas=True)).double() - want).abs() / bound
    print(f"near-identical images: channel differences first {good:.4f} of the bound, lumas subtracted {bad.min().item():.1f} to "
          f"{bad.max().item():.1f} of it")
    assert good <= 1.0 and bool((bad > 1.0).all())


def test_one_step_positions_and_closed_form():
    n, H, W, s, B = R.CASES["long"]
    h, w = R.region("long")
    pos = [h * w - 1 if i is None else i for i in R.STEP_POSITIONS]
    assert [i // R.CHUNK for i in pos] == [0, 0, 1, 64, 65, B - 1] and pos[-1] % R.CHUNK == (h * w - 1) % R.CHUNK
    p, t, closed = R.one_step_pair("fp32")
    assert abs(closed - 108.3495) <= 1e-4
    want = luma_ref.psnr_y(p, t, s, True)
    assert (want - closed).abs().max().item() <= 1e-9
    # a dropped block: +inf; a block counted twice: 3.01 dB less
    assert abs(10.0 * math.log10(2.0) - 3.0103) <= 1e-4
    for name in ("fp16", "bf16"):
        p, t, _ = R.one_step_pair(name)
        codes = (luma_ref.quantise(p, True) - luma_ref.quantise(t, True)) * 255.0
        assert codes.abs().sum().item() == pytest.approx(6.0, abs=1e-9)


def test_finalize_table_is_exact():
    n, H, W, s, B = R.FIN
    for zero in (True, False):
        table, psnr = R.finalize_table(zero)
        assert table.dtype == torch.float32 and table.shape == (n * B,) and psnr.shape == (n,)
        sums = table.view(n, B).double()
        assert torch.equal(sums.sum(dim=1), sums.flip(1).sum(dim=1))    # exact in either order
        assert bool(torch.isinf(psnr[20])) == zero and int(torch.isinf(psnr).sum()) == int(zero)
