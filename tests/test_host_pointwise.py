"""CPU: the pointwise BatchNorm sweep's reference, regime conditions, thresholds and argument checks (tests/pointwise_ref.py).

Nothing here launches a kernel.  The composed float64 reference (the per-entry-point references chained the way the product
chains its launches) is checked against torch.nn.functional.batch_norm + activation under float64 autograd; every exact-regime
case is shown to stay exact (stored values round-trip through bf16 and fp16, every term and partial sum is a dyadic rational
fp32 holds); the thresholds the case table straddles are read from csrc/pointwise.hip; and every entry point's argument checks
are shown to return an error (the calls fail before any launch, so a machine without a GPU can make them)."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import pointwise_ref as R

PKG = "deep-super-resolution_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]
GRAIN = 64.0          # every exact-regime term is a multiple of 1/64


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + "._lib").lib()


def _src():
    return open(os.path.join(ROOT, PKG, "csrc", "pointwise.hip")).read()


# ----------------------------------------------------------------------------- the reference is the contract
def _torch_act(z, act, slope, w):
    if act == R.ACT_NONE:
        return z
    if act == R.ACT_RELU:
        return torch.relu(z)
    if act == R.ACT_LEAKY:
        return TF.leaky_relu(z, slope)
    if act == R.ACT_PRELU:
        return TF.prelu(z, w)
    return {R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid, R.ACT_ELU: TF.elu}[act](z)


@pytest.mark.parametrize("act,slope", R.REAL_ACTS, ids=[R.ACT_NAMES[a] for a, _ in R.REAL_ACTS])
@pytest.mark.parametrize("name", sorted(set(R.REAL_IDS + R.E2E_IDS)))
def test_composed_reference_equals_float64_autograd(name, act, slope):
    """channel_stats -> bn_finalize -> bn_act_fwd and bn_act_bwd_reduce -> bn_bwd_finalize -> bn_act_bwd_apply, as float64
    references, give what F.batch_norm(training) + activation + residual gives under float64 autograd, to 1e-12 of each
    tensor's largest value, on the 16-bit-rounded input (large-mean channels included): the per-entry-point references
    implement the contract and not a private variant.  Pad channels of every result are zero."""
    d = R.real_stream_cached(name, R.BF16)
    c, eps = d["case"]["c"], 1e-5
    got = R.bn_train_act(d["y"], c, d["gamma"], d["beta"], eps, act, slope, d["dout"], d["residual"], rpb=d["case"]["rpb"])
    x = d["y"][:, :c].clone().requires_grad_(True)
    gamma, beta = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    w = torch.tensor([slope], dtype=torch.float64, requires_grad=True)
    out = _torch_act(TF.batch_norm(x, None, None, gamma, beta, True, 0.1, float(torch.tensor(eps, dtype=torch.float32))), act, slope,
                     w) + d["residual"][:, :c]
    out.backward(d["dout"][:, :c])
    pairs = [("out", got["out"][:, :c], out.detach()), ("dx", got["dx"][:, :c], x.grad), ("dgamma", got["dgamma"], gamma.grad),
             ("dbeta", got["dbeta"], beta.grad)]
    if act == R.ACT_PRELU:
        pairs.append(("dprelu", got["dprelu"].reshape(1), w.grad))
    for what, a, b in pairs:
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), (what, float((a - b).abs().max()), float(b.abs().max()))
    if act != R.ACT_SIGMOID:      # sigmoid(0) = 1/2 in a pad channel, by the contract
        assert float(got["out"][:, c:].abs().sum()) == 0.0
    assert float(got["dx"][:, c:].abs().sum()) == 0.0
    for k in ("mean", "rstd", "scale", "shift"):
        assert float(got["fin"][k][c:].abs().sum()) == 0.0
    assert float(got["bw"]["c1"][c:].abs().sum()) == 0.0 and float(got["bw"]["c2"][c:].abs().sum()) == 0.0


def test_reference_finalize_running_statistics_match_torch():
    """bn_finalize's running statistics after `updates` applications == as many F.batch_norm(training) calls (unbiased variance;
    a single element keeps the biased one is checked apart), and bn_eval_affine == F.batch_norm(eval) as an affine map."""
    d = R.real_stream_cached(R.REAL_IDS[1], R.BF16)
    c, cp, p = d["case"]["c"], d["case"]["cp"], d["case"]["p"]
    rm, rv = torch.randn(c, dtype=torch.float64), torch.rand(c, dtype=torch.float64) + 0.5
    fin = R.bn_finalize(R.channel_stats(d["y"], 100), c, cp, float(p), d["gamma"], d["beta"], rm, rv, 5, 0.1, 1e-5, 3)
    trm, trv = rm.clone(), rv.clone()
    m32, e32 = float(torch.tensor(0.1, dtype=torch.float32)), float(torch.tensor(1e-5, dtype=torch.float32))
    for _ in range(3):
        TF.batch_norm(d["y"][:, :c], trm, trv, d["gamma"], d["beta"], True, m32, e32)
    assert torch.allclose(fin["running_mean"], trm, rtol=1e-12, atol=0) and torch.allclose(fin["running_var"], trv, rtol=1e-12, atol=0)
    assert fin["num_batches"] == 8
    assert torch.allclose(fin["var"][:c], d["y"][:, :c].var(0, unbiased=False), rtol=1e-10, atol=0)
    one = R.bn_finalize(R.channel_stats(d["y"][:1], 1), c, cp, 1.0, d["gamma"], d["beta"], rm, rv, 0, 0.1, 1e-5, 1)
    assert torch.allclose(one["running_var"], (1 - m32) * rv, rtol=1e-12, atol=0)          # count == 1: biased variance, 0
    ev = R.bn_eval_affine(d["gamma"], d["beta"], rm, rv, 1e-5, c, cp)
    want = TF.batch_norm(d["y"][:, :c], rm, rv, d["gamma"], d["beta"], False, 0.1, e32)
    assert torch.allclose(d["y"][:, :c] * ev["scale"][:c] + ev["shift"][:c], want, rtol=1e-11, atol=1e-12)


def test_reference_unshuffle_is_pixel_unshuffle():
    for n, h, w, c in R.PIXSHUF_CASES:
        t = torch.randn(n, 2 * h, 2 * w, R.r8(c), dtype=torch.float64)
        want = TF.pixel_unshuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)          # channel 4c + 2i + j
        got = R.unshuffle_nhwc(t, R.r8(4 * c))
        assert torch.equal(got[..., :4 * c], want[..., :4 * c])


def test_number_format_helpers():
    t = torch.tensor([1.0, 1.001, -1.001, 3e-5, 0.0, 1e-45, -300.3], dtype=torch.float64)
    for dtype in (R.BF16, R.F16):
        a, b = R.neighbours(t, dtype)
        lo, hi = torch.minimum(a, b), torch.maximum(a, b)
        assert bool(((lo <= t) & (t <= hi)).all()), (lo, t, hi)
        assert R.representable(a, dtype) and R.representable(b, dtype)
        gap = (hi - lo)
        assert bool(((gap == 0) | (gap == R.ulp16(lo.abs().minimum(hi.abs()), dtype))).all()), (gap, R.ulp16(t, dtype))
        assert bool((gap[[0, 4]] == 0).all()) and bool((gap[[1, 2, 3, 6]] > 0).all())
    assert R.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.75], dtype=torch.float64)).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24]
    assert R.ulp16(torch.tensor([1.0, 300.0], dtype=torch.float64), R.BF16).tolist() == [2.0 ** -7, 2.0]
    assert R.ulp16(torch.tensor([1.0, 300.0], dtype=torch.float64), R.F16).tolist() == [2.0 ** -10, 0.25]


# ----------------------------------------------------------------------------- the exact regime is exact
def _dyadic_sums_exact(terms, rpb, what):
    """Every term is a multiple of 1 / GRAIN and the sum of |terms| of every block, in units of the grain, stays below 2^24: any
    order of fp32 additions (and any FMA contraction) is exact."""
    scaled = terms * GRAIN
    assert torch.equal(scaled, scaled.round()), what
    assert float(R.block_sums(scaled.abs(), rpb).max()) < R.EXACT_LIMIT, what


@pytest.mark.parametrize("name", R.STREAM_IDS)
def test_exact_stream_cases_are_exact(name):
    d = R.exact_stream_cpu(name)
    case = d["case"]
    rpb, c = case["rpb"], case["c"]
    y, dout, res, sc, sh = d["y"], d["dout"], d["residual"], d["scale"], d["shift"]
    for dtype in (R.BF16, R.F16):
        for k in ("y", "dout", "residual"):
            assert R.representable(d[k], dtype), k
    for k in ("scale", "shift", "mean", "rstd", "c1", "c2"):
        assert R.exact_f32(d[k]) and float(d[k][c:].abs().sum()) == 0.0, k
    assert float(y[:, c:].abs().sum()) == 0.0 and float(dout[:, c:].abs().sum()) == 0.0
    _dyadic_sums_exact(y, rpb, "sum y")
    _dyadic_sums_exact(y * y, rpb, "sum y^2")
    for act, slope in R.EXACT_ACTS:
        outs = [R.bn_act_fwd(y, sc, sh, None, act, slope), R.bn_act_fwd(y, sc, sh, res, act, slope), R.bn_act_fwd(y, None, None, res, act, slope),
                R.bn_act_bwd_apply(dout, y, sc, sh, d["mean"], d["rstd"], d["c1"], d["c2"], act, slope, True),
                R.bn_act_bwd_apply(dout, y, sc, sh, d["mean"], d["rstd"], d["c1"], d["c2"], act, slope, False)]
        g, z = R.bn_act_g(dout, y, sc, sh, act, slope)
        for dtype in (R.BF16, R.F16):
            for i, o in enumerate(outs):
                assert R.representable(o, dtype), (R.ACT_NAMES[act], slope, i)
        # the folded coefficients of the apply kernel and each of its three products are exact too
        for t in (sc * d["c2"] * d["rstd"], sc * (d["c2"] * d["mean"] * d["rstd"] - d["c1"]), d["c2"] * d["mean"] * d["rstd"]):
            assert torch.equal(t * GRAIN, (t * GRAIN).round())
        for what, t in (("g", g), ("g*y", g * y), ("dout*z", dout * z), ("z", z)):
            _dyadic_sums_exact(t, rpb, what)
        assert R.exact_f32(R.bn_act_bwd_reduce(dout, y, sc, sh, act, slope, rpb))
    if case["p"] >= 100:      # the case exercises both branches of the activation
        z = y * sc + sh
        assert int((z[:, :c] < 0).sum()) > 10 and int((z[:, :c] > 0).sum()) > 10 and int((z[:, :c] == 0).sum()) > 0


def test_exact_large_cases_and_shifted_sums_are_exact():
    """The capped-grid and non-temporal cases draw the same operands as the streaming cases (integers in [-3, 3], the same
    power-of-two parameters: |term| <= 24, a multiple of 1 / GRAIN), so a block of rpb rows stays exact while 24 * GRAIN * rpb <
    2^24; rpb is what dsr_pw_reduce_blocks gives (at least 64 rows, 1024 blocks).  channel_stats also sums about K = the mean
    of its first four (two, one) rows: a multiple of 1/4, so y - K is one of 1/4 and (y - K)^2 one of 1/16, |.| <= 36."""
    for case in (R.CAPPED, R.NONTEMPORAL):
        rpb = max(64, -(-case["p"] // 1024))
        assert 24 * GRAIN * rpb < R.EXACT_LIMIT and 36 * GRAIN * rpb < R.EXACT_LIMIT
    small = R.exact_stream(dict(R.CAPPED, p=4096, rpb=64, name="capped_sample"))
    assert float(small["y"].abs().max()) == 3 and R.representable(small["y"], R.BF16)
    for name in R.STREAM_IDS:
        d = R.exact_stream_cpu(name)
        y, rpb = d["y"], d["case"]["rpb"]
        for b in range(R.n_blocks(d["case"]["p"], rpb)):
            rows = y[b * rpb:(b + 1) * rpb]
            nk = 4 if len(rows) >= 4 else (2 if len(rows) >= 2 else 1)
            dk = rows - rows[:nk].mean(0)
            _dyadic_sums_exact(dk, len(rows), "sum (y - K)")
            _dyadic_sums_exact(dk * dk, len(rows), "sum (y - K)^2")


def test_exact_act_bwd_and_finalize_cases_are_exact():
    gen = torch.Generator().manual_seed(3)
    for slope in (0.25, 0.5):
        o = R.exact_act_out(gen, (R.PRIME_P, 24), 23, slope)
        dout = R.ints(gen, (R.PRIME_P, 24), 3)
        for dtype in (R.BF16, R.F16):
            assert R.representable(o, dtype)
        for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY, R.ACT_PRELU):
            dy, part = R.act_bwd(dout, o, act, slope, 100)
            assert all(R.representable(dy, dt) for dt in (R.BF16, R.F16)) and R.exact_f32(part)
            _dyadic_sums_exact(dy, 100, "g")
            _dyadic_sums_exact(dout * (o / slope), 100, "prelu terms")
    for rows, cp, stride, _ in R.FINALIZE_CASES:
        part = R.finalize_rows(rows, cp, stride, R.C_OF_CP[cp])
        assert R.exact_f32(part) and float(part.abs().sum(0).max()) < R.EXACT_LIMIT
    for rows, cp, _ in R.BWD_FINALIZE_CASES:
        c = R.C_OF_CP[cp]
        part, mean, rstd = R.bwd_finalize_rows(rows, cp, c)
        got = R.bn_bwd_finalize(part, c, cp, 64.0, mean, rstd)
        assert float(part.abs().sum(0).max()) * 16 < R.EXACT_LIMIT          # |mean| <= 2, rstd <= 2, grain 1/4 . 1/64
        for k in ("dgamma", "dbeta", "c1", "c2"):
            assert R.exact_f32(got[k]), k
        assert R.exact_f32(got["dprelu"].reshape(1))
        assert float(part[:, 2, c:].abs().sum()) > 0 or c == cp          # junk in the pad columns, to be ignored
    for rows, stride, off, c, _, _, scale in R.SUM_ROWS_CASES:
        assert off + c <= stride and rows * 50 * 8 < R.EXACT_LIMIT and scale in (0.125, 0.25, 0.5, 1.0, 2.0)


# ----------------------------------------------------------------------------- the rounded regime stays away from the kinks
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", sorted(set(R.REAL_IDS + R.E2E_IDS)))
def test_rounded_cases_are_well_conditioned(name, dtype):
    """Large-mean and zero-mean channels both present; pre-activations bounded; next to none of them so close to an
    activation's kink that fp32 may see the other sign (those the GPU test lets take either branch); and fewer than 5 % of the
    end-to-end input gradient's elements fall under the 2^-6 floor of its relative check."""
    d = R.real_stream_cached(name, dtype)
    c = d["case"]["c"]
    assert R.representable(d["y"], dtype) and R.representable(d["dout"], dtype) and R.representable(d["residual"], dtype)
    m = d["y"][:, :c].mean(0)
    assert int((m > R.LARGE_MEAN - 1).sum()) >= 1 and int((m.abs() < 1).sum()) >= 1
    for act, slope in R.REAL_ACTS:
        q = R.real_params(d, act, slope, d["case"]["rpb"])
        z = d["y"][:, :c] * q["scale"][:c] + q["shift"][:c]
        assert float(z.abs().max()) < 64
        assert float(R.kink_ambiguous(d["y"], q["scale"], q["shift"], act).double().mean()) < 1e-4
        if name in R.E2E_IDS:
            ref = R.bn_train_act(d["y"], c, d["gamma"], d["beta"], 1e-5, act, slope, d["dout_e2e"], rpb=d["case"]["rpb"])["dx"][:, :c]
            small = ref.abs() <= 2.0 ** -6 * ref.abs().amax(0, keepdim=True)
            assert float(small.double().mean()) < 0.05, (R.ACT_NAMES[act], float(small.double().mean()))


# ----------------------------------------------------------------------------- the thresholds are the ones in the source
def test_thresholds_match_the_source(lib):
    L = importlib.import_module(PKG + "._lib")
    assert (R.BF16, R.F16) == (L.BF16, L.F16)
    assert (R.ACT_NONE, R.ACT_LEAKY, R.ACT_PRELU, R.ACT_RELU, R.ACT_TANH, R.ACT_SIGMOID, R.ACT_ELU) == (
        L.ACT_NONE, L.ACT_LEAKY, L.ACT_PRELU, L.ACT_RELU, L.ACT_TANH, L.ACT_SIGMOID, L.ACT_ELU)
    assert lib.dsr_pw_scratch_rows() == R.SCRATCH_ROWS
    src = _src()

    def define(name):
        return re.search(r"#define\s+%s\s+(\S+(?:\s*<<\s*\d+\))?)" % name, src).group(1)

    assert int(define("DSR_COMPACT_ROWS")) == R.SCRATCH_ROWS
    assert int(define("DSR_FINALIZE_PAR_ROWS")) == R.FINALIZE_PAR_ROWS
    assert int(define("DSR_FINALIZE_PAR_ROWS_BWD")) == R.FINALIZE_PAR_ROWS_BWD
    m = re.fullmatch(r"\((\d+)ull\s*<<\s*(\d+)\)", define("DSR_PW_NT_BYTES"))
    assert int(m.group(1)) << int(m.group(2)) == R.NT_BYTES
    # the literal thresholds of the launchers (compared with all white space removed: a reformat is no change)
    flat = re.sub(r"\s+", "", src)
    for line in ("if(rows<=%d){" % R.SERIAL_ROWS, "rows>=%d?DSR_COMPACT_ROWS:16" % R.COMPACT_WIDE_ROWS,
                 "tiles>%d&&tiles<=DSR_FINALIZE_PAR_ROWS" % R.SERIAL_ROWS, "tiles>%d&&Cp%%16==0" % R.FINALIZE_PAR16_ROWS,
                 "blocks>%d&&blocks<=DSR_FINALIZE_PAR_ROWS_BWD&&(!dprelu||Cp<=64)" % R.SERIAL_ROWS,
                 "rows>%d&&rows<=DSR_FINALIZE_PAR_ROWS&&row_stride>1" % R.SERIAL_ROWS, "cap=nt?16384:%d;" % R.GRID_CAP):
        assert line in flat, line
    hdr = open(os.path.join(ROOT, PKG, "csrc", "dsr_kernels.h")).read()
    assert "(Cp)%%8==0&&(Cp)<=%d)" % R.CP_MAX in re.sub(r"\s+", "", hdr)


def test_case_table_straddles_every_threshold():
    for entry, (rows, thresholds) in R.partial_row_thresholds().items():
        for t in thresholds:
            assert t in rows and t + 1 in rows, (entry, t)
        assert 1 in rows
    fin = R.FINALIZE_CASES
    assert {1, 7, 8, 32, 33, 128, 129, 512, 513, 4095, 4096} <= {r for r, *_ in fin}
    assert any(r == 129 and cp % 16 == 0 for r, cp, *_ in fin) and any(r == 129 and cp == 24 for r, cp, *_ in fin)
    assert any(stride > cp for _, cp, stride, _ in fin)
    bwd = R.BWD_FINALIZE_CASES
    assert {1, 3, 4, 32, 33, 64, 65} <= {r for r, *_ in bwd}
    assert {(40, 64, True), (40, 64, False), (40, 136, True)} <= set(bwd)
    srw = R.SUM_ROWS_CASES
    assert any(s == 1 for _, s, *_ in srw) and {c for *_, c, _, _ in srw} == {0, 1} and {a for *_, a, _ in srw} == {0, 1}
    assert any(off > 0 for _, _, off, *_ in srw)
    # every thread mapping, with C one less than Cp where a chunk is ragged
    assert [R.rpi_of(cp) for cp in R.CP_LIST] == [256, 85, 32, 15, 1]
    assert 256 % (24 // 8) == 1 and 256 % (136 // 8) == 1          # one idle thread each
    assert R.C_OF_CP[24] == 23 and R.C_OF_CP[136] == 135
    for cp in R.CP_LIST:
        rpi = R.rpi_of(cp)
        ps = {c["p"] for c in R.STREAM_CASES if c["cp"] == cp}
        assert {1, rpi + 1, 2 * rpi + 1, R.PRIME_P} <= ps and (rpi <= 2 or rpi - 1 in ps)
        assert any(c["p"] % c["rpb"] and c["p"] > c["rpb"] for c in R.STREAM_CASES if c["cp"] == cp)      # a short last block
    # the capped grid iterates its two-row loop and runs its tail; the non-temporal case is just over the size threshold
    p, rpi = R.CAPPED["p"], R.CAPPED["rpi"]
    assert (p + rpi - 1) // rpi > R.GRID_CAP and p > 2 * R.GRID_CAP * rpi and p < 3 * R.GRID_CAP * rpi
    assert R.CAPPED["p"] * R.CAPPED["cp"] * 2 < R.NT_BYTES
    assert R.NT_BYTES <= R.NONTEMPORAL["p"] * R.NONTEMPORAL["cp"] * 2 < R.NT_BYTES + (1 << 20)
    assert any(4 * R.r8(c) != R.r8(4 * c) for *_, c in R.PIXSHUF_CASES) and any(4 * R.r8(c) == R.r8(4 * c) for *_, c in R.PIXSHUF_CASES)


# ----------------------------------------------------------------------------- argument checks: an error, and no launch
def test_argument_checks(lib):
    """A null required pointer, Cp % 8 != 0, Cp > 2048, PReLU without its weight pointer, a LeakyReLU slope <= 0 in act_bwd and
    empty shapes return DSR_E_ARG with a message.  Valid-looking pointers are host memory: the checks come before any launch."""
    buf = (C.c_float * 64)()
    a = C.c_void_p(C.addressof(buf))
    N, st = None, None
    PR, LK, NO = R.ACT_PRELU, R.ACT_LEAKY, R.ACT_NONE
    calls = []

    def each_null(fn, args, ptr_slots, tail=()):
        for i in ptr_slots:
            calls.append(lambda i=i: fn(*[N if j == i else v for j, v in enumerate(args)], *tail))

    def each_cp(fn, args, cp_slot):
        for bad in (0, 12, 20, R.CP_MAX + 8, -8):
            calls.append(lambda bad=bad: fn(*[bad if j == cp_slot else v for j, v in enumerate(args)]))

    fwd = [R.BF16, a, a, a, a, a, 16, 8, NO, 0.0, N, st]
    each_null(lib.dsr_pw_bn_act_fwd, fwd, (1, 5))
    each_cp(lib.dsr_pw_bn_act_fwd, fwd, 7)
    calls += [lambda: lib.dsr_pw_bn_act_fwd(R.BF16, a, a, N, a, a, 16, 8, NO, 0.0, N, st),          # scale without shift
              lambda: lib.dsr_pw_bn_act_fwd(R.BF16, a, N, a, a, a, 16, 8, NO, 0.0, N, st),
              lambda: lib.dsr_pw_bn_act_fwd(R.BF16, a, a, a, a, a, 16, 8, PR, 0.0, N, st),          # PReLU without its pointer
              lambda: lib.dsr_pw_bn_act_fwd(7, a, a, a, a, a, 16, 8, NO, 0.0, N, st),               # dtype
              lambda: lib.dsr_pw_bn_act_fwd(R.BF16, a, a, a, a, a, 0, 8, NO, 0.0, N, st)]           # P == 0
    red = [R.F16, a, a, a, a, a, a, 16, 8, 1, 16, NO, 0.0, N, a, st]
    each_null(lib.dsr_pw_bn_act_bwd_reduce, red, (1, 2, 3, 4, 5, 6, 14))
    each_cp(lib.dsr_pw_bn_act_bwd_reduce, red, 8)
    calls += [lambda: lib.dsr_pw_bn_act_bwd_reduce(R.F16, a, a, a, a, a, a, 16, 8, 1, 16, PR, 0.0, N, a, st),
              lambda: lib.dsr_pw_bn_act_bwd_reduce(R.F16, a, a, a, a, a, a, 16, 8, 0, 16, NO, 0.0, N, a, st),      # no blocks
              lambda: lib.dsr_pw_bn_act_bwd_reduce(R.F16, a, a, a, a, a, a, 16, 8, 1, 0, NO, 0.0, N, a, st)]       # rpb == 0
    app = [R.BF16, a, a, a, a, a, a, a, a, a, 16, 8, NO, 0.0, N, 1, st]
    each_null(lib.dsr_pw_bn_act_bwd_apply, app, (1, 2, 3, 4, 5, 6, 7, 8, 9))
    each_cp(lib.dsr_pw_bn_act_bwd_apply, app, 11)
    calls.append(lambda: lib.dsr_pw_bn_act_bwd_apply(R.BF16, a, a, a, a, a, a, a, a, a, 16, 8, PR, 0.0, N, 1, st))
    ab = [R.BF16, a, a, a, 1, 4, 4, 8, 8, 0, NO, 0.0, N, 1, 16, a, st]
    each_null(lib.dsr_pw_act_bwd, ab, (1, 2, 3))
    each_cp(lib.dsr_pw_act_bwd, ab, 7)
    calls += [lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 4, 8, 8, 0, PR, 0.0, N, 1, 16, a, st),
              lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 4, 8, 8, 0, LK, 0.0, N, 1, 16, a, st),           # slope 0
              lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 4, 8, 8, 0, LK, -0.25, N, 1, 16, a, st),
              lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 4, 8, 8, 0, LK, float("nan"), N, 1, 16, a, st),
              lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 4, 8, 7, 0, NO, 0.0, N, 1, 16, a, st),           # odd CoP
              lambda: lib.dsr_pw_act_bwd(R.BF16, a, a, a, 1, 4, 0, 8, 8, 0, NO, 0.0, N, 1, 16, a, st)]
    for fn in (lib.dsr_pw_channel_stats, lib.dsr_pw_colsum):
        cs = [R.BF16, a, 16, 8, 1, 16, a, st]
        each_null(fn, cs, (1, 6))
        each_cp(fn, cs, 3)
        calls.append(lambda fn=fn: fn(R.BF16, a, 0, 8, 1, 16, a, st))
    fin = [a, 4, 8, 8, 8, 4.0, a, a, a, a, a, 0.1, 1e-5, 1, a, a, a, a, st]
    each_null(lib.dsr_pw_bn_finalize, fin, (0, 6, 7, 14, 15, 16, 17))
    calls += [lambda: lib.dsr_pw_bn_finalize(a, 0, 8, 8, 8, 4.0, a, a, a, a, a, 0.1, 1e-5, 1, a, a, a, a, st),     # no rows
              lambda: lib.dsr_pw_bn_finalize(a, 4, 8, 9, 8, 4.0, a, a, a, a, a, 0.1, 1e-5, 1, a, a, a, a, st),     # C > Cp
              lambda: lib.dsr_pw_bn_finalize(a, 4, 7, 8, 8, 4.0, a, a, a, a, a, 0.1, 1e-5, 1, a, a, a, a, st),     # stride < Cp
              lambda: lib.dsr_pw_bn_finalize(a, 4, 8, 8, 8, 0.0, a, a, a, a, a, 0.1, 1e-5, 1, a, a, a, a, st),     # count 0
              lambda: lib.dsr_pw_bn_finalize(a, 4, 8, 8, 8, 4.0, a, a, a, a, a, 0.1, 1e-5, -1, a, a, a, a, st)]
    bfin = [a, 4, 8, 8, 4.0, a, a, a, a, a, a, a, st]
    each_null(lib.dsr_pw_bn_bwd_finalize, bfin, (0, 5, 6, 10, 11))
    calls += [lambda: lib.dsr_pw_bn_bwd_finalize(a, 0, 8, 8, 4.0, a, a, a, a, a, a, a, st),
              lambda: lib.dsr_pw_bn_bwd_finalize(a, 4, 9, 8, 4.0, a, a, a, a, a, a, a, st),
              lambda: lib.dsr_pw_bn_bwd_finalize(a, 4, 8, 8, 0.0, a, a, a, a, a, a, a, st)]
    sr = [a, 4, 8, 0, 8, 1.0, a, 0, 1, st]
    each_null(lib.dsr_pw_sum_rows, sr, (0, 6))
    calls += [lambda: lib.dsr_pw_sum_rows(a, -1, 8, 0, 8, 1.0, a, 0, 1, st), lambda: lib.dsr_pw_sum_rows(a, 4, 0, 0, 8, 1.0, a, 0, 1, st),
              lambda: lib.dsr_pw_sum_rows(a, 4, 8, -1, 8, 1.0, a, 0, 1, st), lambda: lib.dsr_pw_sum_rows(a, 4, 8, 0, 0, 1.0, a, 0, 1, st)]
    ev = [a, a, a, a, 1e-5, 8, 8, a, a, a, a, st]
    each_null(lib.dsr_pw_bn_eval_affine, ev, (0, 1, 2, 3, 7, 8))
    calls += [lambda: lib.dsr_pw_bn_eval_affine(a, a, a, a, 1e-5, 9, 8, a, a, a, a, st),
              lambda: lib.dsr_pw_bn_eval_affine(a, a, a, a, 1e-5, 0, 8, a, a, a, a, st)]
    nc = [R.BF16, a, a, a, 1, 3, 4, 4, 8, NO, st]
    each_null(lib.dsr_pw_act_bwd_nchw, nc, (1, 2, 3))
    calls += [lambda: lib.dsr_pw_act_bwd_nchw(R.BF16, a, a, a, 1, 3, 4, 4, 12, NO, st),            # Cp % 8
              lambda: lib.dsr_pw_act_bwd_nchw(R.BF16, a, a, a, 1, 9, 4, 4, 8, NO, st)]             # Cp < C
    each_null(lib.dsr_pw_add, [R.BF16, a, a, a, 4, st], (1, 2, 3))
    calls.append(lambda: lib.dsr_pw_add(R.BF16, a, a, a, 0, st))
    calls.append(lambda: lib.dsr_pw_reduce_blocks(100, None))
    assert len(calls) > 100
    for i, call in enumerate(calls):
        rc = call()
        assert rc == -1, f"call #{i} returned {rc}"
        assert lib.dsr_last_error(), i
