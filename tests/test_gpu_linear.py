"""GPU: exact-integer / float64 parity sweep of the dense-head kernels of csrc/linear.hip through the raw C ABI, in bf16 and fp16
(references, operand generators and case tables: linear_ref.py; the references against float64 torch, the exactness of the
regimes, the tie counts, the launcher branches the table reaches and the Adam floor: test_host_linear.py).

Regime A: integer operands, every partial sum below 2^24 in any order -> every output must EQUAL the float64 reference, bit for
bit (a reference sum is normalised to +0; the kernels' accumulators start from +0 too).  Regime B: larger integers, the 16-bit
outputs must be round-to-nearest-even of the exact value.  Data movement (flatten, cast16) is compared on the bit patterns.
Two comparisons carry a bound, both measured in the test and printed: the fused Adam against the float64 model
(max(1e-6, 4 x torch's own fp32 deviation), the bar of test_clipped_adam_against_float64_reference) and dense2's sigmoid
(max(4 x torch's fp32 deviation, 2) fp32 ulp).  Every output and workspace of every call sits inside a sentinel-filled buffer
(canaries.py) whose margins are checked after every case; what a kernel must leave alone must still hold the sentinel."""
import ctypes as C
import importlib

import pytest
import torch

import clip_ref
import linear_ref as R
from adam_args import adam_args
from canaries import Canaries

pytestmark = pytest.mark.gpu

PKG = "deep-super-resolution_amd"
BOTH = (R.BF16, R.F16)
DT = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]
INT_OF = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


def same_bits(got, want, what, zero_sign_free=False):
    """Equality of the bit patterns (got: device tensor; want: tensor of the same dtype, host or device).  zero_sign_free: a
    zero may carry either sign (only where linear_ref.py says so); every other value is still compared bit for bit."""
    want = want.to(got.device)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if zero_sign_free:
        got, want = torch.where(got == 0, torch.zeros_like(got), got), torch.where(want == 0, torch.zeros_like(want), want)
    if torch.equal(bits(got), bits(want)):
        return
    bad = (bits(got) != bits(want)).nonzero()
    i = tuple(bad[0].tolist())
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ; first at {bad[:6].tolist()}: got {got[i].item()!r} "
                         f"want {want[i].item()!r}")


class Calls:
    """The entry points, every output inside a canary buffer.  Operands stay alive until the canaries are checked."""

    def __init__(self, dev, dtype=R.BF16):
        self.L = P("_lib")
        self.lib = self.L.lib()
        self.dev, self.dtype, self.tdt = dev, dtype, R.DTYPES[dtype]
        self.can = Canaries(dev)
        self.keep = []

    def fresh(self):
        """New canaries for the next case (the previous ones have been checked)."""
        self.can, self.keep = Canaries(self.dev), []

    def up16(self, t):
        """float64 -> the 16-bit storage type on the device; the values must be representable."""
        out = R.to16(t, self.dtype)
        assert bool((out.to(R.F64) == t).all()), "operand not representable"
        return self.hold(out)

    def up32(self, t):
        out = t.to(torch.float32)
        assert bool((out.to(R.F64) == t.to(R.F64)).all()), "operand not representable"
        return self.hold(out)

    def hold(self, t):
        t = t.contiguous().to(self.dev)
        self.keep.append(t)
        return t

    def out(self, shape, dtype, what, fill=None):
        o = self.can.alloc(shape, dtype, what)
        if fill is not None:
            o.fill_(fill)
        return o

    def call(self, name, *args):
        self.L.check(getattr(self.lib, "dsr_" + name)(*args, stream()))


# ----------------------------------------------------------------------------- dsr_linear_fwd
@pytest.mark.parametrize("K", R.FWD_K)
def test_linear_fwd_exact(dev, K):
    """Regime A and the impulse form at every (B, O) of fwd_shapes(K), both storage types, bias null / non-null, no activation,
    LeakyReLU 0.25 (exact) and 0.2 (one fp32 product): the fp32 output EQUALS the reference; the split-K workspace is exactly
    dsr_linear_fwd_workspace() bytes between sentinels."""
    for B, O in R.fwd_shapes(K):
        for impulse in (False, True):
            if impulse and O * K > R.IMPULSE_MAX:
                continue
            x, w, bias = R.fwd_case(B, O, K, impulse)
            pre = R.linear_pre(x, w)
            for dtype in BOTH:
                k = Calls(dev, dtype)
                xd, wd, bd = k.up16(x), k.up16(w), k.up32(bias)
                wsz = k.lib.dsr_linear_fwd_workspace(B, K, O)
                todo = []
                for bv, bp in ((None, None), (bias, bd)):
                    for act, slope in R.SLOPES:
                        ws = k.out((wsz // 4,), torch.float32, "fwd workspace")
                        out = k.out((B, O), torch.float32, "fwd out", float("nan"))
                        k.call("linear_fwd", dtype, ptr(xd), ptr(wd), ptr(bp), act, slope, ptr(out), B, K, O, ptr(ws), wsz)
                        todo.append((out, R.linear_fwd(x, w, bv, act, slope, pre), f"fwd {(B, O, K)} dtype {dtype} impulse {impulse} "
                                     f"bias {bv is not None} act {act} slope {slope}"))
                k.can.check()
                for out, want, what in todo:
                    same_bits(out, want.to(torch.float32), what)


# ----------------------------------------------------------------------------- dsr_linear_dgrad
def _dgrad(k, dy, w, B, O, K, what):
    dx = k.out((B, K), k.tdt, what, float("nan"))
    k.call("linear_dgrad", k.dtype, ptr(dy), ptr(w), ptr(dx), B, O, K)
    return dx


@pytest.mark.parametrize("K", R.DG_K)
def test_linear_dgrad_exact_and_rounded(dev, K):
    """Regime A (dx equals the exact sum), the impulse form and regime B (dx is the round-to-nearest-even of the exact sum, ties
    included) at every (B, O) of dgrad_shapes(K); dx is pre-filled with NaN and none may survive."""
    for B, O in R.dgrad_shapes(K):
        for dtype in BOTH:
            k = Calls(dev, dtype)
            todo = []
            for regime, impulse in (("A", False), ("A", True), ("B", False)):
                if impulse and O * K > R.IMPULSE_MAX:
                    continue
                dy, w = R.dgrad_case(B, O, K, regime, dtype, impulse)
                want = R.linear_dgrad(dy, w)
                what = f"dgrad {(B, O, K)} dtype {dtype} regime {regime} impulse {impulse}"
                if regime == "A":
                    assert R.fits16(want), what
                todo.append((_dgrad(k, k.up16(dy), k.up16(w), B, O, K, what), R.to16(want, dtype), what))
            k.can.check()
            for dx, want, what in todo:
                assert not bool(dx.isnan().any()), what + ": a NaN survived"
                same_bits(dx, want, what)


@pytest.mark.parametrize("dtype", DT)
def test_linear_dgrad_wide_form(dev, dtype, monkeypatch):
    """DSR_LINEAR_DGRAD_COLS=256 (read per call) takes the 256-column instantiation from K = 256 * 512 on: K = 131072 and 131080
    run it, K = 131064 must still take the 128-column form.  With and without the switch the result equals the reference, hence
    each other."""
    O = R.DG_WIDE_O
    for K in R.DG_WIDE_K:
        for B in (16, 33):
            k = Calls(dev, dtype)
            dy, w = R.dgrad_case(B, O, K, "B", dtype)
            want = R.to16(R.linear_dgrad(dy, w), dtype)
            dyd, wd = k.up16(dy), k.up16(w)
            monkeypatch.delenv("DSR_LINEAR_DGRAD_COLS", raising=False)
            narrow = _dgrad(k, dyd, wd, B, O, K, "dgrad 128 columns")
            monkeypatch.setenv("DSR_LINEAR_DGRAD_COLS", "256")
            wide = _dgrad(k, dyd, wd, B, O, K, "dgrad 256 columns")
            monkeypatch.delenv("DSR_LINEAR_DGRAD_COLS", raising=False)
            k.can.check()
            for got, what in ((narrow, "128"), (wide, "256")):
                assert not bool(got.isnan().any()), (B, K, what)
                same_bits(got, want, f"dgrad {(B, O, K)} switch {what}")
            same_bits(wide, narrow, f"dgrad {(B, O, K)} wide against narrow")


# ----------------------------------------------------------------------------- dsr_linear_wgrad / _gathered
@pytest.mark.parametrize("Bp", R.WG_BP)
@pytest.mark.parametrize("dtype", DT)
def test_linear_wgrad_exact(dev, dtype, Bp):
    """Every (O, K) of the table: the plain form, the gathered form at R = 1, scale = 1 (bit-equal to the plain one) and at an
    (R, scale) pair rotating through R 1-4 and scale 1, 1/2, 1/4 (exact) and 1/3 (one fp32 product), and the impulse form."""
    i = 0
    for O in R.WG_O:
        for K in R.WG_K:
            k = Calls(dev, dtype)
            todo = []
            dyT, xT = R.wgrad_case(Bp, O, K)
            a, b = k.up16(dyT), k.up16(xT)
            plain = k.out((O, K), torch.float32, "wgrad dw", float("nan"))
            k.call("linear_wgrad", dtype, ptr(a), ptr(b), ptr(plain), Bp, O, K)
            g1 = k.out((O, K), torch.float32, "gathered dw", float("nan"))
            k.call("linear_wgrad_gathered", dtype, ptr(a), ptr(b), ptr(g1), Bp, O, K, 1, 1.0)
            want = R.linear_wgrad(dyT, xT).to(torch.float32)
            todo += [(plain, want, "plain"), (g1, want, "gathered R 1")]
            Rr, scale = R.WG_RS[i % len(R.WG_RS)]
            i += 1
            for impulse in (False, True):
                dyT, xT = R.wgrad_case(Bp, O, K, Rr, impulse)
                a, b = k.up16(dyT), k.up16(xT)
                g = k.out((O, K), torch.float32, "gathered dw", float("nan"))
                k.call("linear_wgrad_gathered", dtype, ptr(a), ptr(b), ptr(g), Bp, O, K, Rr, scale)
                todo.append((g, R.linear_wgrad(dyT, xT, scale).to(torch.float32), f"gathered R {Rr} scale {scale} impulse {impulse}"))
            if K % 4 == 0:
                dyT, xT = R.wgrad_case(Bp, O, K, 1, True)
                g = k.out((O, K), torch.float32, "wgrad dw", float("nan"))
                k.call("linear_wgrad", dtype, ptr(k.up16(dyT)), ptr(k.up16(xT)), ptr(g), Bp, O, K)
                todo.append((g, R.linear_wgrad(dyT, xT).to(torch.float32), "plain impulse"))
            k.can.check()
            for got, want, what in todo:
                same_bits(got, want, f"wgrad Bp {Bp} {(O, K)} dtype {dtype} {what}")


# ----------------------------------------------------------------------------- dsr_linear_wgrad_adam, every mode of dsr_adam_args
class AdamRun:
    """One set of p / m / v / shadow buffers with three sentinel rows below row O, and the launches that update them."""

    def __init__(self, k, O, K, shadow=True):
        self.k, self.O, self.K = k, O, K
        p0, m0, v0 = R.adam_state(O, K)
        self.full = [k.out((O + 3, K), torch.float32, n) for n in ("p", "m", "v")]
        self.full_sh = k.out((O + 3, K), torch.bfloat16, "shadow") if shadow else None
        for t, t0 in zip(self.full, (p0, m0, v0)):
            t[:O].copy_(t0)
        self.p, self.m, self.v = (t[:O] for t in self.full)
        self.sh = self.full_sh[:O] if shadow else None

    def state(self):
        return [self.p, self.m, self.v] + ([self.sh] if self.sh is not None else [])

    def snapshot(self):
        return [t.clone() for t in self.state()]

    def rows_below_untouched(self, what):
        for t in self.full + ([self.full_sh] if self.full_sh is not None else []):
            assert self.k.can.untouched(t[self.O:]), what + ": a row o >= O was written"


def _args(step, gs, hyper=None, loss_scale=None, found_inf=None):
    """dsr_adam_args of the sweep: R.ADAM's constants, the mode given by which of the three device words are set."""
    A = R.ADAM
    return adam_args(step, A["lr"], A["b1"], A["b2"], A["eps"], gs, hyper, loss_scale, found_inf)


def _two_launch(k, a, b, Bp, O, K, Rr, scale, run, step, gs, hyper=None, loss_scale=None, found_inf=None):
    g = k.out((O, K), torch.float32, "g", float("nan"))
    if Rr == 1 and scale == 1.0:
        k.call("linear_wgrad", k.dtype, ptr(a), ptr(b), ptr(g), Bp, O, K)
    else:
        k.call("linear_wgrad_gathered", k.dtype, ptr(a), ptr(b), ptr(g), Bp, O, K, Rr, scale)
    k.call("pw_adam", ptr(run.p), ptr(g), ptr(run.m), ptr(run.v), O * K, ptr(run.sh), _args(step, gs, hyper, loss_scale, found_inf))


def _fused(k, a, b, Bp, O, K, Rr, scale, run, step, gs, hyper=None, loss_scale=None, found_inf=None):
    k.call("linear_wgrad_adam", k.dtype, ptr(a), ptr(b), Bp, O, K, Rr, scale, ptr(run.p), ptr(run.m), ptr(run.v), ptr(run.sh),
           _args(step, gs, hyper, loss_scale, found_inf))


def _kpb(monkeypatch, kpb):
    if kpb is None:
        monkeypatch.delenv("DSR_WGRAD_ADAM_KPB", raising=False)
    else:
        monkeypatch.setenv("DSR_WGRAD_ADAM_KPB", kpb)


@pytest.mark.parametrize("Bp", R.WG_BP)
@pytest.mark.parametrize("dtype", DT)
def test_wgrad_adam_equals_two_launches_and_float64(dev, dtype, Bp, monkeypatch):
    """dsr_linear_wgrad_adam at every case of wa_cases() (every (O, K); R, step, DSR_WGRAD_ADAM_KPB and a power-of-two grad_scale
    rotating), with and without
    the bf16 shadow: p, m, v and the shadow are BIT-EQUAL to dsr_linear_wgrad(_gathered) + dsr_pw_adam on the same inputs, for
    every R and scale (1, 1/2 and the inexact 1/3); rows o >= O keep the sentinel; the shadow is exactly p.to(bfloat16); and
    p is within the Adam bar -- max(1e-6, 4 x torch.optim.Adam's fp32 CPU deviation from the float64 model), relative 2-norm --
    of clip_ref.ClippedAdam in float64 fed the exact gradient; m and v likewise against that model with the betas rounded to
    fp32, which is how the C ABI receives them (against the nominal betas v is 6.5e-6 off: 1 - fl32(0.999) is not 0.001).
    Printed: the largest floor and error; measured on the MI355X: floor 4.2e-8 -> bar 1e-6, largest error 3.9e-8."""
    A = R.ADAM
    worst_floor = worst_err = 0.0
    for Rr, O, K, t, gs, kpb in R.wa_cases():
        _kpb(monkeypatch, kpb)
        scale = R.WA_SCALE[Rr]
        k = Calls(dev, dtype)
        dyT, xT = R.wgrad_case(Bp, O, K, Rr)
        a, b = k.up16(dyT), k.up16(xT)
        step = k.hold(torch.tensor([t], dtype=torch.int32))
        what = f"wgrad_adam dtype {dtype} Bp {Bp} kpb {kpb} R {Rr} {(O, K)} step {t} grad_scale {gs}"
        two = AdamRun(k, O, K)
        _two_launch(k, a, b, Bp, O, K, Rr, scale, two, step, gs)
        runs = [AdamRun(k, O, K, True), AdamRun(k, O, K, False)]
        for run in runs:
            _fused(k, a, b, Bp, O, K, Rr, scale, run, step, gs)
        k.can.check()
        for run in runs:
            run.rows_below_untouched(what)
            for got, want, name in zip(run.state(), two.state(), "pmvs"):
                same_bits(got, want, f"{what}: {name} against the two-launch path (shadow {run.sh is not None})")
        same_bits(runs[0].sh, runs[0].p.to(torch.bfloat16), what + ": shadow is not p.to(bfloat16)")
        # float64 model and torch's fp32 floor on the same inputs: p with the nominal betas (the project's bar), m and v with the
        # betas as the C ABI carries them (fp32: 1 - fl32(0.999) is 1.3e-5 off 0.001, which no fp32-argument kernel can undo)
        g = R.linear_wgrad(dyT, xT, scale)
        p0, m0, v0 = R.adam_state(O, K)
        for betas, names in (((A["b1"], A["b2"]), "p"), ((R.f32(A["b1"]), R.f32(A["b2"])), "mv")):
            ref = clip_ref.ClippedAdam([p0.numpy()], lr=A["lr"], betas=betas, eps=A["eps"], grad_scale=gs)
            ref.m[0], ref.v[0], ref.t = m0.double().numpy(), v0.double().numpy(), t - 1
            ref.step([g.numpy()])
            tp = dict(zip("pmv", R.adam_torch_fp32(p0, m0, v0, g * gs, t, A["lr"], betas[0], betas[1], A["eps"])))
            want = dict(zip("pmv", (ref.p[0], ref.m[0], ref.v[0])))
            got = dict(zip("pmv", runs[0].state()))
            for name in names:
                floor = R.rel(tp[name], want[name])
                bar = max(1e-6, 4 * floor)
                err = R.rel(got[name].cpu(), want[name])
                worst_floor, worst_err = max(worst_floor, floor), max(worst_err, err)
                assert err <= bar, f"{what}: {name} err {err:.3e} floor {floor:.3e} bar {bar:.3e}"
    print(f"\nfused Adam vs float64: largest torch-fp32 floor {worst_floor:.3e} -> bar {max(1e-6, 4 * worst_floor):.3e}; "
          f"largest error {worst_err:.3e}")


@pytest.mark.parametrize("Bp", R.WG_BP)
@pytest.mark.parametrize("dtype", DT)
def test_wgrad_adam_hyper_write_discipline(dev, dtype, Bp, monkeypatch):
    """dsr_linear_wgrad_adam with the hyper block at every case of wa_cases(), with and without the shadow: hyper[1] = 1 gives the
    bits of the plain mode; hyper[1] = 0.5 the bits of dsr_linear_wgrad(_gathered) + dsr_pw_adam in that mode; loss_scale = 4 on gradients
    times 4 the bits of the unscaled run (a power of two: exact); found_inf = 1 leaves p, m, v and the shadow bit-identical;
    rows o >= O keep the sentinel throughout."""
    A = R.ADAM
    for Rr, O, K, t, gs, kpb in R.wa_cases():
        _kpb(monkeypatch, kpb)
        scale = R.WA_SCALE[Rr]
        k = Calls(dev, dtype)
        dyT, xT = R.wgrad_case(Bp, O, K, Rr)
        a, b, a4 = k.up16(dyT), k.up16(xT), k.up16(dyT * 4.0)
        step = k.hold(torch.tensor([t], dtype=torch.int32))
        h1 = k.hold(torch.tensor([A["lr"], 1.0], dtype=torch.float32))
        h5 = k.hold(torch.tensor([A["lr"], 0.5], dtype=torch.float32))
        four, one, zero = (k.hold(torch.tensor([v], dtype=torch.float32)) for v in (4.0, 1.0, 0.0))
        what = f"wgrad_adam with hyper dtype {dtype} Bp {Bp} kpb {kpb} R {Rr} {(O, K)} step {t} grad_scale {gs}"
        for shadow in (True, False):
            plain, hy1, hy5, two5, ls4, ls0, inf = (AdamRun(k, O, K, shadow) for _ in range(7))
            _fused(k, a, b, Bp, O, K, Rr, scale, plain, step, gs)
            _fused(k, a, b, Bp, O, K, Rr, scale, hy1, step, gs, h1)
            _fused(k, a, b, Bp, O, K, Rr, scale, hy5, step, gs, h5, None, zero)
            _two_launch(k, a, b, Bp, O, K, Rr, scale, two5, step, gs, h5, None, zero)
            _fused(k, a4, b, Bp, O, K, Rr, scale, ls4, step, gs, h5, four)          # grad_scale is replaced by 1 / loss_scale
            _fused(k, a, b, Bp, O, K, Rr, scale, ls0, step, 1.0, h5)
            before = inf.snapshot()
            _fused(k, a, b, Bp, O, K, Rr, scale, inf, step, gs, h5, four, one)
            k.can.check()
            for run in (plain, hy1, hy5, two5, ls4, ls0, inf):
                run.rows_below_untouched(what)
            for name, x, y, z, u, v, w, f, f0 in zip("pmvs", plain.state(), hy1.state(), hy5.state(), two5.state(), ls4.state(),
                                                     ls0.state(), inf.state(), before):
                same_bits(y, x, f"{what}: {name}, hyper[1] = 1 against the non-hyper form")
                same_bits(z, u, f"{what}: {name}, hyper[1] = 0.5 against the two-launch hyper path")
                same_bits(v, w, f"{what}: {name}, loss_scale 4 on gradients x 4 against the unscaled run")
                same_bits(f, f0, f"{what}: {name} written although found_inf is set")
            assert not torch.equal(bits(hy5.p), bits(plain.p)), what + ": the clipping coefficient changed nothing"
            k.fresh()


def _smallest_wa_cases():
    """The two smallest (O, K) of wa_cases() (O = 1: not a multiple of the 64-row tile), with their R, step, grad_scale, kpb."""
    return sorted(R.wa_cases(), key=lambda c: c[1] * c[2])[:2]


@pytest.mark.parametrize("Bp", R.WG_BP)
@pytest.mark.parametrize("dtype", DT)
def test_wgrad_adam_scaler_without_hyper_block(dev, dtype, Bp, monkeypatch):
    """The one mode of dsr_adam_args without an ancestor on the dense launch: loss_scale and found_inf set, hyper NULL.
    loss_scale = 4, found_inf = 0 on gradients built 4 x too large is BIT-EQUAL in p, m, v and the shadow to the plain mode with
    grad_scale = 0.25 on the same inputs (1 / 4 is exact); found_inf = 1 with NaN in both factors leaves all four tensors and the
    sentinel rows below row O bit-identical.  With and without the shadow."""
    for Rr, O, K, t, gs, kpb in _smallest_wa_cases():
        _kpb(monkeypatch, kpb)
        scale = R.WA_SCALE[Rr]
        k = Calls(dev, dtype)
        dyT, xT = R.wgrad_case(Bp, O, K, Rr)
        a4, b = k.up16(dyT * 4.0), k.up16(xT)
        nan_a, nan_b = (k.hold(torch.full_like(t16, float("nan"))) for t16 in (a4, b))
        step = k.hold(torch.tensor([t], dtype=torch.int32))
        four, one, zero = (k.hold(torch.tensor([v], dtype=torch.float32)) for v in (4.0, 1.0, 0.0))
        what = f"wgrad_adam scaler-only dtype {dtype} Bp {Bp} kpb {kpb} R {Rr} {(O, K)} step {t}"
        for shadow in (True, False):
            plain, amp, inf = (AdamRun(k, O, K, shadow) for _ in range(3))
            _fused(k, a4, b, Bp, O, K, Rr, scale, plain, step, 0.25)
            _fused(k, a4, b, Bp, O, K, Rr, scale, amp, step, 1.0, None, four, zero)
            before = inf.snapshot()
            _fused(k, nan_a, nan_b, Bp, O, K, Rr, scale, inf, step, 1.0, None, four, one)
            k.can.check()
            for run in (plain, amp, inf):
                run.rows_below_untouched(what)
            for name, x, y, f, f0 in zip("pmvs", plain.state(), amp.state(), inf.state(), before):
                same_bits(y, x, f"{what}: {name}, loss_scale 4 against the plain mode with grad_scale 0.25")
                same_bits(f, f0, f"{what}: {name} written although found_inf is set")
            assert not torch.equal(bits(plain.p), bits(before[0])), what + ": the plain run moved nothing"
            k.fresh()


def _scaler_modes(dev):
    """(hyper, loss_scale, found_inf): the scaler alone, and the scaler with a hyper block."""
    four, zero = (torch.tensor([v], dtype=torch.float32, device=dev) for v in (4.0, 0.0))
    h5 = torch.tensor([R.ADAM["lr"], 0.5], dtype=torch.float32, device=dev)
    return ((None, four, zero), (h5, four, None))


@pytest.mark.parametrize("Bp", R.WG_BP)
@pytest.mark.parametrize("dtype", DT)
def test_grad_scale_is_ignored_under_a_scaler(dev, dtype, Bp, monkeypatch):
    """loss_scale = 4 with grad_scale = 123 gives the bits of loss_scale = 4 with grad_scale = 1, with and without the hyper
    block, on the dense launch: the two smallest cases, with and without the shadow."""
    modes = _scaler_modes(dev)
    for Rr, O, K, t, gs, kpb in _smallest_wa_cases():
        _kpb(monkeypatch, kpb)
        scale = R.WA_SCALE[Rr]
        k = Calls(dev, dtype)
        dyT, xT = R.wgrad_case(Bp, O, K, Rr)
        a, b = k.up16(dyT), k.up16(xT)
        step = k.hold(torch.tensor([t], dtype=torch.int32))
        what = f"grad_scale under a scaler dtype {dtype} Bp {Bp} R {Rr} {(O, K)}"
        for shadow in (True, False):
            for mode in modes:
                r1, r123 = AdamRun(k, O, K, shadow), AdamRun(k, O, K, shadow)
                before = r1.snapshot()
                _fused(k, a, b, Bp, O, K, Rr, scale, r1, step, 1.0, *mode)
                _fused(k, a, b, Bp, O, K, Rr, scale, r123, step, 123.0, *mode)
                k.can.check()
                for name, x, y in zip("pmvs", r1.state(), r123.state()):
                    same_bits(y, x, f"{what}: {name}, dense launch, hyper {mode[0] is not None}")
                assert not torch.equal(bits(r1.p), bits(before[0])), what
            k.fresh()


def test_grad_scale_is_ignored_under_a_scaler_pointwise(dev):
    """The same on the per-tensor and the multi-tensor launch, over 3 ragged tensors of 1, 4097 and 1027 (= 3 mod 4) elements."""
    modes = _scaler_modes(dev)
    k = Calls(dev)
    step = k.hold(torch.tensor([3], dtype=torch.int32))
    gen = torch.Generator().manual_seed(77)
    sizes = (1, 4097, 1027)
    gs = [k.hold(torch.randn(n, generator=gen)) for n in sizes]
    for mode in modes:
        state = {}
        for launch in ("one", "multi"):
            for grad_scale in (1.0, 123.0):
                gen.manual_seed(78)
                ps, ms, vs = ([k.out((n,), torch.float32, w) for n in sizes] for w in "pmv")
                for p_, m_, v_ in zip(ps, ms, vs):
                    p_.copy_(torch.randn(p_.numel(), generator=gen))
                    m_.copy_(0.1 * torch.randn(p_.numel(), generator=gen))
                    v_.copy_(0.5 + torch.rand(p_.numel(), generator=gen))
                p0 = [p_.clone() for p_ in ps]
                blk = _args(step, grad_scale, *mode)
                if launch == "one":
                    for p_, g_, m_, v_ in zip(ps, gs, ms, vs):
                        k.call("pw_adam", ptr(p_), ptr(g_), ptr(m_), ptr(v_), p_.numel(), None, blk)
                else:
                    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
                    k.call("pw_adam_multi", len(sizes), tab(ps), tab(gs), tab(ms), tab(vs), (C.c_size_t * len(sizes))(*sizes), blk)
                k.can.check()
                assert all(not torch.equal(bits(x), bits(y)) for x, y in zip(ps, p0)), launch
                state[launch, grad_scale] = ps + ms + vs
            for x, y in zip(state[launch, 1.0], state[launch, 123.0]):
                same_bits(y, x, f"grad_scale under a scaler: {launch} launch, hyper {mode[0] is not None}")


@pytest.mark.parametrize("mode", ["scaler", "clip"])
def test_empty_parameter_is_a_no_op_in_every_mode(dev, mode):
    """optim.FusedAdam over [p0 of 0 elements, p1 of 5 elements], each with a gradient, takes three steps under a
    DynamicLossScaler and under max_grad_norm = 1.0 without raising, and leaves p1 bit-equal to the same run without p0: an empty
    parameter is a no-op in every mode."""
    O = P("optim")
    gen = torch.Generator().manual_seed(11)
    w1 = torch.randn(5, generator=gen)
    grads = [torch.randn(5, generator=gen) * 3.0 for _ in range(3)]            # norm > 1: the clipping coefficient bites

    def run(with_empty):
        p1 = w1.clone().to(dev).requires_grad_(True)
        ps = ([torch.zeros(0, device=dev, requires_grad=True)] if with_empty else []) + [p1]
        opt = O.FusedAdam(ps, lr=1e-2, max_grad_norm=1.0 if mode == "clip" else None)
        scaler = O.DynamicLossScaler(init_scale=4.0) if mode == "scaler" else None
        for g in grads:
            for p in ps:
                p.grad = torch.zeros(0, device=dev) if p.numel() == 0 else (g * (4.0 if scaler else 1.0)).to(dev)
            if scaler:
                scaler.step(opt)
                scaler.update()
            else:
                opt.step()
        assert opt.step_t.item() == 3
        return p1.detach()

    alone, beside = run(False), run(True)
    assert not torch.equal(alone.cpu(), w1)
    same_bits(beside, alone, f"p1 beside an empty parameter, {mode}")


# ----------------------------------------------------------------------------- dsr_linear_factor_gram
@pytest.mark.parametrize("dtype", DT)
def test_factor_gram_is_the_integer_norm(dev, dtype):
    """Integer factors in [-3, 3]: every Gram partial is an integer below 2^24 and every fp64 product sum below 2^53, so the sum
    of the dots EQUALS scale^2 |dW|_F^2 computed in int64 from the materialised product; N = R Bp over every nsub and CG > 1;
    two calls leave bit-identical workspaces, which are exactly dsr_linear_factor_gram_workspace() bytes between sentinels."""
    for Bp, Rr, O, K, scale in R.gram_cases():
        k = Calls(dev, dtype)
        dyT, xT = R.wgrad_case(Bp, O, K, Rr)
        a, b = k.up16(dyT), k.up16(xT)
        wsz = k.lib.dsr_linear_factor_gram_workspace(Bp, O, K, Rr)
        nd = k.lib.dsr_linear_factor_gram_dots(Bp, Rr)
        assert wsz > 0 and wsz % 4 == 0 and nd == (Rr * Bp) ** 2 // 16
        ws = [k.out((wsz // 4,), torch.float32, "gram workspace") for _ in range(2)]
        for w in ws:
            k.call("linear_factor_gram", dtype, ptr(a), ptr(b), Bp, O, K, Rr, scale, ptr(w), wsz)
        k.can.check()
        what = f"gram dtype {dtype} Bp {Bp} R {Rr} {(O, K)} scale {scale}"
        same_bits(ws[0], ws[1], what + ": two calls differ")
        dots = ws[0][:2 * nd].cpu().view(torch.float64)
        norm2 = R.gram_norm2(dyT, xT)
        assert norm2 < 2 ** 53
        got = float(dots.sum())
        assert got == float(norm2) * scale * scale, f"{what}: sum of dots {got!r}, scale^2 |dW|^2 {float(norm2) * scale * scale!r}"


# ----------------------------------------------------------------------------- dsr_dense2_bwd / dsr_dense2_fwd
@pytest.mark.parametrize("dtype", DT)
def test_dense2_bwd_exact_and_rounded(dev, dtype):
    """B x Bp (32, 40, 64 where >= B) x K1, slope 0.25, h with +0 and -0 (derivative 1 at both).  Regime A: dw2, db2, db1 equal
    the reference (sums: -0 == +0) and dy16 / dyT16 its bit patterns (a zero product may carry either sign); regime B: the fp32 outputs still equal it, the 16-bit ones
    are its round-to-nearest-even.  dy16 has exactly B rows, dyT16 columns b >= B are zero: the sentinels follow directly."""
    for B in R.D2B_B:
        for Bp in R.D2B_BP:
            if Bp < B:
                continue
            for K1 in R.D2B_K1:
                k = Calls(dev, dtype)
                todo = []
                for regime in "AB":
                    dout, out, h, w2 = R.dense2_bwd_case(B, K1, regime)
                    ref = R.dense2_bwd(dout, out, h, w2, Bp, R.D2_SLOPE)
                    if regime == "A":
                        assert R.fits16(ref["dy"])
                    o = {"dw2": k.out((K1,), torch.float32, "dw2"), "db2": k.out((1,), torch.float32, "db2"),
                         "db1": k.out((K1,), torch.float32, "db1"), "dy": k.out((B, K1), k.tdt, "dy16"),
                         "dyT": k.out((K1, Bp), k.tdt, "dyT16")}
                    k.call("dense2_bwd", dtype, ptr(k.up32(dout)), ptr(k.up32(out)), ptr(k.up32(h)), ptr(k.up32(w2)), B, K1, Bp,
                           R.D2_SLOPE, ptr(o["dw2"]), ptr(o["db2"]), ptr(o["db1"]), ptr(o["dy"]), ptr(o["dyT"]))
                    todo.append((o, ref, f"dense2_bwd dtype {dtype} B {B} Bp {Bp} K1 {K1} regime {regime}"))
                k.can.check()
                for o, ref, what in todo:
                    for name in ("dw2", "db2", "db1"):
                        got = o[name].cpu().to(R.F64)
                        assert torch.equal(got, ref[name]), f"{what}: {name} got {got[:8].tolist()} want {ref[name][:8].tolist()}"
                    same_bits(o["dy"], R.to16(ref["dy"], dtype), what + ": dy16", zero_sign_free=True)
                    same_bits(o["dyT"], R.to16(ref["dyT"], dtype), what + ": dyT16", zero_sign_free=True)
                    assert not bool(o["dyT"][:, B:].any()), what + ": dyT16 pad columns"


def test_dense2_fwd_sigmoid(dev):
    """Integer h, w2, b2: the pre-sigmoid sum is exact in any order.  Sum 0 -> exactly 0.5; |sum| >= 20 (saturated in fp32, up to
    +-200 where expf overflows): finite, in [0, 1], exactly 1 for sum >= 20; every other sum within max(4 d, 2) fp32 ulp of the
    float64 sigmoid, d = torch's fp32 CPU sigmoid's own deviation on the same sums.  Measured on the MI355X (printed by this test):
    d = 0.868 ulp -> bar 3.471 ulp; the kernel's largest deviation over the 235 unsaturated sums is 0.868 ulp."""
    k = Calls(dev)
    todo = []
    for B in R.D2F_B:
        for K1 in R.D2F_K1:
            for offset in (range(7) if B == 1 else (0,)):
                h, w2, b2, tgt = R.dense2_fwd_case(B, K1, offset)
                out = k.out((B,), torch.float32, "dense2 out", float("nan"))
                k.call("dense2_fwd", ptr(k.up32(h)), ptr(k.up32(w2)), ptr(k.hold(torch.tensor([b2], dtype=torch.float32))), B, K1, ptr(out))
                todo.append((out, tgt, (B, K1, offset)))
    k.can.check()
    sums = torch.cat([t for _, t, _ in todo])
    got = torch.cat([o.cpu() for o, _, _ in todo]).to(R.F64)
    assert bool(got.isfinite().all()) and bool(((got >= 0) & (got <= 1)).all())
    assert bool((got[sums == 0] == 0.5).all()) and int((sums == 0).sum()) >= 10
    assert bool((got[sums >= R.SATURATED] == 1.0).all())
    assert {100.0, -100.0, 200.0, -200.0} <= set(sums.tolist())
    mid = sums.abs() < R.SATURATED
    d, bar = R.sigmoid_bar(sums[mid])
    ref = torch.sigmoid(sums[mid])
    err = ((got[mid] - ref).abs() / R.ulp32(ref))
    print(f"\ndense2 sigmoid: torch fp32 deviation {d:.3f} ulp -> bar {bar:.3f} ulp; kernel's largest deviation {float(err.max()):.3f} ulp "
          f"over {int(mid.sum())} sums")
    worst = int(err.argmax())
    assert float(err.max()) <= bar, f"sum {float(sums[mid][worst])}: got {float(got[mid][worst])!r} ref {float(ref[worst])!r}"


# ----------------------------------------------------------------------------- dsr_cast16
@pytest.mark.parametrize("dtype", DT)
def test_cast16_equals_torch(dev, dtype):
    """dst equals tensor.to(dtype) bit for bit (NaN: NaN-ness, not payload) on ties both ways, signed zeros, subnormals, Inf, NaN,
    the fp16 overflow edge (65504, 65519.99, 65520) and the bf16 one; n = 8, 2040, 2048, 2056, and one n just above
    8 * 256 * 8192 elements, where the capped grid strides (data and reference on the device)."""
    k = Calls(dev, dtype)
    todo = []
    for n in R.CAST_N:
        x = R.cast_case(n)
        dst = k.out((n,), k.tdt, "cast16 dst")
        k.call("cast16", dtype, ptr(k.hold(x)), ptr(dst), n)
        todo.append((dst, x.to(k.tdt), n))
    n = R.CAST_GRID_CAP + 8 * 257
    g = torch.Generator(device=dev).manual_seed(n)
    big = torch.randn(n, generator=g, device=dev, dtype=torch.float32) * 300.0
    sp = R.cast_specials().to(dev)
    big[-len(sp):] = sp
    big[R.CAST_GRID_CAP - 4:R.CAST_GRID_CAP + 4] = sp[:8]
    dst = k.out((n,), k.tdt, "cast16 dst")
    k.call("cast16", dtype, ptr(big), ptr(dst), n)
    todo.append((dst, big.to(k.tdt), n))
    k.can.check()
    for dst, want, n in todo:
        want = want.to(dev)
        nan = want.isnan()
        assert torch.equal(dst.isnan(), nan), f"cast16 n {n}: NaN-ness"
        same_bits(torch.where(nan, torch.zeros_like(dst), dst), torch.where(nan, torch.zeros_like(want), want), f"cast16 n {n} dtype {dtype}")


# ----------------------------------------------------------------------------- dsr_flatten
@pytest.mark.parametrize("switch", [pytest.param(None, id="tile"), pytest.param("0", id="strided")])
@pytest.mark.parametrize("dtype", DT)
def test_flatten_moves_every_element(dev, dtype, switch, monkeypatch):
    """A 16-bit counter pattern through modes 0, 1 (Bp 32 and 64 where >= B) and 2 at every shape of flatten_shapes(), with
    DSR_FLATTEN_TILE unset and 0: mode 0 writes exactly B x C x HW elements (nothing for pad channels), mode 1 pads the batch with
    zero columns, mode 2 writes zero pad channels, and mode2(mode0(x)) == x on the real channels."""
    if switch is None:
        monkeypatch.delenv("DSR_FLATTEN_TILE", raising=False)
    else:
        monkeypatch.setenv("DSR_FLATTEN_TILE", switch)
    forms = set()
    for B, HW, Cc, Cp in R.flatten_shapes():
        k = Calls(dev, dtype)
        act = R.counter((B, HW, Cp), start=B + HW)
        flat = R.counter((B, Cc * HW), start=3 * Cp)
        actd, flatd = k.hold(act.view(k.tdt)), k.hold(flat.view(k.tdt))
        todo = []
        o0 = k.out((B, Cc * HW), k.tdt, "flatten mode 0")
        k.call("flatten", dtype, ptr(actd), ptr(o0), B, HW, Cc, Cp, 0, 0)
        todo.append((o0, R.flatten0(act, Cc), "mode 0"))
        back = k.out((B, HW, Cp), k.tdt, "flatten mode 2 of mode 0")
        k.call("flatten", dtype, ptr(o0), ptr(back), B, HW, Cc, Cp, 0, 2)
        rt = act.clone()
        rt[:, :, Cc:] = 0
        todo.append((back, rt, "mode 2 of mode 0"))
        o2 = k.out((B, HW, Cp), k.tdt, "flatten mode 2")
        k.call("flatten", dtype, ptr(flatd), ptr(o2), B, HW, Cc, Cp, 0, 2)
        todo.append((o2, R.flatten2(flat, Cc, HW, Cp), "mode 2"))
        forms.add(R.takes_tile_form(0, HW, Cp, 0, switch))
        for Bp in R.FL_BP:
            if Bp < B:
                continue
            o1 = k.out((Cc * HW, Bp), k.tdt, "flatten mode 1")
            k.call("flatten", dtype, ptr(actd), ptr(o1), B, HW, Cc, Cp, Bp, 1)
            todo.append((o1, R.flatten1(act, Cc, Bp), f"mode 1 Bp {Bp}"))
            forms.add(R.takes_tile_form(1, HW, Cp, Bp, switch))
        k.can.check()
        for got, want, what in todo:
            same_bits(got, want.view(k.tdt), f"flatten {(B, HW, Cc, Cp)} dtype {dtype} switch {switch} {what}")
    assert forms == ({True, False} if switch is None else {False})
