"""CPU: what tests/test_gpu_compact_sweep.py relies on, without a device -- every case of tests/compact_sweep_ref.py is in the
regime it claims (partial rows, pixels per row and empty rows derived from dsr_pw_prelu_c_rows of the built library; pixel lanes
and idle threads of each channel layout; thread counts of the elementwise launches against the grid cap and the 2^31 limit); the
exact operands are exact; an fp32 emulation of the slope gradient in the kernel's own order equals the yardstick on the integer
data and sits inside the band on the float data; and the wrong variants -- a dropped last partial row, a row counted twice, a
`z >= 0` branch, the mask taken from the output under a negative slope -- are outside the band or unequal on the exact data."""
import importlib

import pytest
import torch

import compact_ref as R
import compact_sweep_ref as S

PKG = "deep-super-resolution_amd"
DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def lib():
    P("_build").build()
    yield P("_lib").lib()
    S.clear()


# ----------------------------------------------------------------------------- regimes
def test_backward_pixel_counts_reach_the_cap_and_the_empty_rows(lib):
    assert lib.dsr_pw_prelu_c_fold_width() == S.FOLD_W
    geo = {}
    for p in S.BWD_PIXELS:
        rows = lib.dsr_pw_prelu_c_rows(p)
        assert rows == S.rows_of(p)
        geo[p] = S.geometry(p, 64, rows)
    a, b, c = (geo[p] for p in S.BWD_PIXELS)
    # exactly on the cap: 1024 rows of 64 pixels, one more pixel would not get a row of its own
    assert (a["rows"], a["ppr"], a["empty"], a["last"]) == (S.MAX_ROWS, S.MIN_PIX, 0, S.MIN_PIX)
    assert lib.dsr_pw_prelu_c_rows(S.BWD_PIXELS[0] - 1) == S.MAX_ROWS and lib.dsr_pw_prelu_c_rows(S.BWD_PIXELS[0] - S.MIN_PIX) == S.MAX_ROWS - 1
    # one pixel past it: ppr grows to 65, rows 1009..1023 own nothing, row 1008 holds 17 pixels
    assert (b["rows"], b["ppr"], b["used"], b["empty"], b["last"]) == (S.MAX_ROWS, 65, 1009, 15, 17)
    assert b["used"] * b["ppr"] >= S.BWD_PIXELS[1] > (b["used"] - 1) * b["ppr"]
    # three times the cap: several pixels per pixel lane, and still empty rows at the end
    assert (c["rows"], c["ppr"]) == (S.MAX_ROWS, 193) and c["per_thread"] == 7 > 1 and c["empty"] == 5 and 0 < c["last"] < c["ppr"]
    for g in (a, b, c):
        assert g["npl"] == 32 and g["idle"] == 0 and g["fold_adds"] == 16
    # what tests/test_gpu_compact.py reaches: 65 rows of 64 pixels (66 at the 4161 pixels of the 2048-channel layout here)
    p = S.FOLD_W * S.MIN_PIX + 1
    assert p == 4097 and lib.dsr_pw_prelu_c_rows(p) == S.FOLD_W + 1 and S.geometry(p, 64)["ppr"] == 64
    assert lib.dsr_pw_prelu_c_rows(4161) == 66


def test_channel_layouts_reach_idle_threads_and_one_pixel_lane(lib):
    want = {(8, 8): (256, 0, 1), (20, 24): (85, 1, 1), (70, 72): (28, 4, 1), (2048, 2048): (1, 0, 8)}
    for (c, cp), (npl, idle, turns) in want.items():
        assert (c, cp) in S.LAYOUTS and 8 <= cp <= 2048 and cp % 8 == 0 and c <= cp
        for p in S.layout_pixels(c, cp):
            g = S.geometry(p, cp, lib.dsr_pw_prelu_c_rows(p))
            assert (g["npl"], g["idle"], g["fold_turns"]) == (npl, idle, turns), (c, cp, p)
            assert g["npl"] * g["chunks"] * 4 * 8 <= 64 * 1024                 # the block's LDS table
            assert 18 * p < 2 ** 24
    assert 256 % 3 != 0 and 256 % 9 != 0 and (20 < 24) and (70 < 72)           # chunk counts that do not divide 256; pad channels
    assert S.layout_pixels(*S.WIDE) == [130, 4161] and S.geometry(130, 2048)["rows"] == 3 and S.geometry(4161, 2048)["rows"] == 66
    assert 65537 in S.layout_pixels(8, 8) and S.geometry(65537, 8)["empty"] == 15
    # with 256 pixel lanes and 65 pixels a row most lanes are idle in their only turn; with 28 lanes a lane takes three
    assert S.geometry(65537, 8)["per_thread"] == 1 and S.geometry(65537, 72)["per_thread"] == 3
    assert len(S.bwd_cases()) == len(set(S.bwd_cases())) == 3 + 3 * 2 + 2


def test_forward_and_shuffle_shapes_pass_the_grid_cap(lib):
    for c, cp, p in S.FWD_CAP_CASES:
        nvec = p * cp // 8
        threads, turns = S.grid_threads(nvec)
        assert nvec > S.GRID_THREADS == 2097152 and threads == S.GRID_THREADS and turns == 2, (c, cp, p)
    for s, (n, c, h, w) in S.SHUFFLE_FWD_LARGE + [S.SHUFFLE_NULL_FWD_LARGE]:
        total = n * c * h * w * s * s
        assert S.GRID_THREADS < total < S.ELEM_LIMIT and S.grid_threads(total)[1] == 2, (s, total)
    for s, (n, c, h, w) in S.SHUFFLE_BWD_LARGE + [S.SHUFFLE_NULL_BWD_LARGE]:
        total = n * c * h * w                                             # one thread per LR pixel of a plane
        assert S.GRID_THREADS < total and total * s * s < S.ELEM_LIMIT and S.grid_threads(total)[1] == 2, (s, total)
    for n, c, h, w in S.SHUFFLE_SMALL:
        for s in (1, 2, 3, 4):
            assert 256 < n * c * h * w < S.GRID_THREADS and n * c * h * w * s * s < S.GRID_THREADS
    assert 2 * 3 * 5 * 7 < 256                                            # the shape of tests/test_gpu_compact.py: one block
    assert S.SHUFFLE_NULL_SMALL[1] in S.SHUFFLE_SMALL


# ----------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("c,cp,p", [(64, 64, 65537), (20, 24, 4097), (2048, 2048, 130)])
def test_exact_operands_are_exact_in_every_type(c, cp, p):
    case = S.exact_case(c, p)
    for key in ("z", "dy", "y", "dz"):
        assert R.representable(case[key], R.BF16) and R.representable(case[key], R.F16), key
    assert R.representable(case["slope"], R.BF16) and float(case["slope"].min()) < 0 and bool((case["slope"] == 0).any())
    assert float((case["dy"] * case["z"]).abs().sum(dim=0).max()) <= 18 * p < 2 ** 24
    assert torch.equal(case["dslope"].float().double(), case["dslope"])
    assert float(case["z"].min()) == -6 and float(case["z"].max()) == 6 and bool((case["z"] == 0).any())
    assert torch.equal(S.row_sums(case, p, cp).sum(dim=0), case["dslope"])
    assert len(set(case["slope"][:9].tolist())) == min(9, c)


@pytest.mark.parametrize("c,cp,p", [(64, 64, 65536), (64, 64, 65537), (64, 64, 3 * 65536 + 5), (20, 24, 65537), (70, 72, 4097),
                                    (2048, 2048, 130)])
def test_emulation_equals_the_yardstick_on_exact_data_and_wrong_variants_do_not(c, cp, p):
    case = S.exact_case(c, p)
    geo = S.geometry(p, cp)
    want = case["dslope"]
    assert torch.equal(S.emulate_dslope(case, p, cp).double(), want)
    live = S.row_sums(case, p, cp)[geo["used"] - 1] != 0                # channels to which the last used row contributes
    dropped = S.emulate_dslope(case, p, cp, drop_last_row=True).double()
    assert bool(live.any()) and bool((dropped != want)[live].all())
    twice = S.emulate_dslope(case, p, cp, double_row=0).double()
    assert not torch.equal(twice, want)
    # z >= 0 as the branch: dz differs at every z == 0 under a slope other than one (dslope cannot tell: its term there is 0)
    z, dy, sl = case["z"], case["dy"], case["slope"].view(1, -1)
    dz_ge = torch.where(z >= 0, dy, dy * sl)
    assert not torch.equal(dz_ge, case["dz"]) and torch.equal(dz_ge[z != 0], case["dz"][z != 0])
    # the mask taken from the output: wrong under a negative slope, in dz and in dslope
    wz, wslope = R.prelu_bwd(S.nchw(dy), S.nchw(z), case["slope"], from_output=True)
    neg = case["slope"] < 0
    assert not torch.equal(S.flat(wz), case["dz"]) and bool((wslope != want)[neg].any())
    assert torch.equal(S.flat(wz)[:, ~neg], case["dz"][:, ~neg])


# ----------------------------------------------------------------------------- float data
@pytest.mark.parametrize("p", S.FLOAT_PIXELS)
@pytest.mark.parametrize("dtype", DT)
def test_emulation_is_inside_the_band_and_wrong_variants_outside(lib, dtype, p):
    case = S.float_case(dtype, p)
    rows = lib.dsr_pw_prelu_c_rows(p)
    geo = S.geometry(p, 64, rows)
    assert geo["depth"] == geo["per_thread"] + 32 + 16 + 6 == {65537: 57, 3 * 65536 + 5: 61}[p]
    bound = S.band(p, 64, case["mag"], rows)
    want = case["dslope"]
    assert bool((bound > 0).all())
    ratio = S.worst_ratio(S.emulate_dslope(case, p, 64), want, bound)
    print(f"dslope float {dtype} P={p}: fp32 emulation, worst |emulation - f64| / band = {ratio:.4f} (depth {geo['depth']})")
    assert ratio <= 1.0
    dropped = (S.emulate_dslope(case, p, 64, drop_last_row=True).double() - want).abs() / bound
    twice = (S.emulate_dslope(case, p, 64, double_row=3).double() - want).abs() / bound
    print(f"  dropped last row: {float(dropped.min()):.1f} .. {float(dropped.max()):.1f} of the band; "
          f"row counted twice: {float(twice.min()):.1f} .. {float(twice.max()):.1f}")
    assert float(dropped.median()) > 1.0 and float(dropped.max()) > 10.0
    assert float(twice.median()) > 1.0 and float(twice.max()) > 10.0
    _, wslope = R.prelu_bwd(S.nchw(case["dy"]), S.nchw(case["z"]), case["slope"], from_output=True)
    neg = case["slope"] < 0
    assert int(neg.sum()) > 10 and bool((((wslope - want).abs() / bound)[neg] > 1.0).all())
    # `z >= 0` cannot show here (no z is 0): the exact data above is what catches it
    assert not bool((case["z"] == 0).any())


# ----------------------------------------------------------------------------- shuffle-add
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_shuffle_yardsticks_are_exact_and_tell_a_swap(s):
    case = S.shuffle_case(s, S.SHUFFLE_SMALL[0])
    for key in ("out", "out_nobase", "dt", "dbase"):
        assert torch.equal(case[key].float().double(), case[key]), key
    assert float(case["dbase"].abs().max()) <= 50 * s * s
    assert not torch.equal(case["out"], case["out_nobase"])
    if s > 1:
        assert not torch.equal(R.shuffle_add(case["t"], case["base"], s, swap=True), case["out"])
