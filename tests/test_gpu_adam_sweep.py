"""GPU: elementwise float64 sweep of the Adam kernels through the raw C ABI -- dsr_pw_adam (adam_stream: vector body, u = 0 / 1
halves, scalar tail, bf16 shadow, the second pass of the grid-stride loop) and dsr_pw_adam_multi (chunks, groups of 64, views
off a 16-byte boundary) -- against tests/adam_sweep_ref.py: single steps from a given state, every element inside the bands
derived there, the all-zero regime and the shadow bit for bit, guard words round every tensor, g unmodified.

dsr_pw_adam takes 16-byte aligned operands only (8 for the shadow); every view handed to it here lies on such a boundary, and
the refused calls are made on a build that has first shown, with found_inf set so that no kernel could touch a tensor, that it
refuses them."""
import ctypes as C
import importlib

import pytest
import torch

import adam_sweep_ref as R
from adam_args import adam_args
from canaries import Canaries

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"


def P(sub):
    return importlib.import_module(PKG + "." + sub)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    P("_lib").lib()
    return torch.device("cuda:0")


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def block(case, dev, keep):
    """dsr_adam_args of the case's mode; the device words it points to go into `keep`."""
    mode = case.mode
    f32 = lambda *x: torch.tensor(x, dtype=torch.float32, device=dev)
    step = torch.tensor([case.t], dtype=torch.int32, device=dev)
    kw = dict(lr=case.lr, b1=case.b1, b2=case.b2, eps=case.eps, grad_scale=mode["grad_scale"])
    if mode.get("hyper"):
        kw.update(hyper=f32(case.lr, R.COEF), lr=123.0)            # with a hyper block the block's own lr must not be read
    if "loss_scale" in mode:
        kw["loss_scale"] = f32(mode["loss_scale"])
    if "found_inf" in mode:
        kw["found_inf"] = f32(mode["found_inf"])
    keep += [step] + [x for x in kw.values() if isinstance(x, torch.Tensor)]
    return adam_args(step, **kw)


SHADOW_FILL = 12345.0


class State:
    """p, g, m, v (and a shadow) of a case on the device, each operand in its own guarded arena."""

    def __init__(self, case, data, dev, aligned=False):
        self.case, self.data = case, data
        off = lambda k: [0 if aligned else o[k] for o in case.offs]
        self.a = [R.Arena([d[k] for d in data], off(k), dev) for k in range(4)]
        self.sh = None
        if case.shadow:
            self.sh = R.Arena([torch.full((d[0].numel(),), SHADOW_FILL, dtype=torch.bfloat16, device=dev) for d in data],
                              [0] * len(data), dev)
        self.g0 = self.a[1].snapshot()

    def views(self, i):
        return [a.views[i] for a in self.a]

    def tables(self):
        k = len(self.data)
        return [(C.c_void_p * k)(*[v.data_ptr() for v in a.views]) for a in self.a] + \
               [(C.c_size_t * k)(*[d[0].numel() for d in self.data])]

    def check(self):
        """Bands, zero regime, shadow, guards, g.  Returns the worst |delta| / band of p, m, v over the case."""
        torch.cuda.synchronize()
        worst = [0.0, 0.0, 0.0]
        for i, (p, g, m, v, r) in enumerate(self.data):
            got = self.views(i)
            got = (got[0], got[2], got[3])
            if not p.is_cuda:
                got = tuple(x.cpu() for x in got)
            rp, rm, rv, zok = R.compare(got, (p, g, m, v), r, self.case.hyp())
            assert zok, (self.case, i, "all-zero regime: p must keep its bits, m' = v' = +0")
            for j, x in enumerate((rp, rm, rv)):
                w = float(x.max())
                worst[j] = max(worst[j], w)
                assert w <= 1.0, (self.case, f"tensor {i} of {p.numel()} elements", "pmv"[j], w, int(x.argmax()),
                                  int((x > 1.0).sum()), R.REGIMES[int(r[int(x.argmax())])])
            if self.sh is not None:
                want = R.bf16_bits(self.views(i)[0])
                bad = self.sh.views[i].view(torch.int16) != want
                assert not bool(bad.any()), (self.case, i, "shadow", int(bad.sum()), int(bad.nonzero()[0]))
        for a, what in zip(self.a + ([self.sh] if self.sh else []), "pgmvs"):
            assert a.guards_intact(), (self.case, what)
        assert self.a[1].unchanged(self.g0), (self.case, "g was written")
        print(f"{self.case!r}: worst |delta|/band  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
        return worst


def launch_pw(st8, i, args):
    L = P("_lib")
    p, g, m, v = st8.views(i)
    for x in (p, g, m, v):
        assert x.data_ptr() % 16 == 0
    sh = st8.sh.views[i] if st8.sh else None
    assert sh is None or sh.data_ptr() % 8 == 0
    L.check(L.lib().dsr_pw_adam(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(sh), args, stream()))


def launch_multi(st8, args):
    L = P("_lib")
    tp, tg, tm, tv, ns = st8.tables()
    L.check(L.lib().dsr_pw_adam_multi(len(st8.data), tp, tg, tm, tv, ns, args, stream()))


# ----------------------------------------------------------------------------- 1: dsr_pw_adam over the size list
@pytest.mark.parametrize("case", R.PW_CASES, ids=repr)
def test_pw_adam_sweep(dev, case):
    """Every size of the list -- the tail alone, one vector, n/4 = 256 and 257 (the edge of the u = 1 half), one block, the
    second block, 512 blocks -- with and without the shadow, modes / steps / sets rotated so that every (mode, step) pair occurs.
    Observed on the MI355X: see test_past_the_grid_cap's docstring for the figures of this file."""
    keep = []
    s = State(case, R.case_data(case), dev)
    launch_pw(s, 0, block(case, dev, keep))
    s.check()


# ----------------------------------------------------------------------------- 2: dsr_pw_adam_multi over the four tables
@pytest.mark.parametrize("case", R.MT_CASES, ids=repr)
def test_multi_adam_sweep(dev, case):
    """Tables of 1, 64, 65 and 129 tensors (one, one, two and three launches), the 11-block tensor at slots 0, 63 and 64, every
    one of p, g, m, v independently 0, 4, 8 or 12 bytes off a 16-byte boundary."""
    keep = []
    s = State(case, R.case_data(case), dev)
    launch_multi(s, block(case, dev, keep))
    s.check()


# ----------------------------------------------------------------------------- 3: the two launches agree bit for bit
@pytest.mark.parametrize("k", [0, 7, 13, 22, 18])
def test_multi_and_per_tensor_launch_agree_bit_for_bit(dev, k):
    """The same aligned inputs through dsr_pw_adam_multi and through one dsr_pw_adam per tensor: both run adam_update with
    contraction off behind the same adam_coef, so p, m and v agree in every bit (guard words included)."""
    sizes = list(R.MT_SIZES) + [3, 5, 7, 1028, 2047, 2052, 13317]
    case = R.Case(f"cross{k}", sizes, k, seed=3000 + k)
    data = R.case_data(case)
    keep = []
    a, b = State(case, data, dev, aligned=True), State(case, data, dev, aligned=True)
    args = block(case, dev, keep)
    launch_multi(a, args)
    for i in range(len(sizes)):
        launch_pw(b, i, args)
    torch.cuda.synchronize()
    for x, y, what in zip(a.a, b.a, "pgmv"):
        diff = x.buf != y.buf
        assert not bool(diff.any()), (case, what, int(diff.sum()))
    a.check()


# ----------------------------------------------------------------------------- 4: past the grid cap
def test_past_the_grid_cap(dev):
    """n = 134 220 807 = 65536 * 2048 + 2048 + 1024 + 4 + 3 with the shadow at t = 1000: the grid is capped at 65536 blocks, so the
    grid-stride loop runs a second pass in which block 0 does both halves, block 1 a full u = 0 half and one u = 1 vector; the
    tail is 3.  Inputs are generated on the device, and adam_step and its bands are evaluated there in float64 with torch's
    elementwise ops (test_host_adam_sweep.py pins that function on the CPU).  About 16 GB of HBM, freed at the end.

    Observed on the MI355X: zero of 134 220 807 elements outside, worst |delta| / band p 0.992, m 0.648, v 0.333; 0.4 s.
    The rest of this file: dsr_pw_adam over the size list p <= 0.987 (final rounding of p), m <= 0.633, v <= 0.330 -- case
    for case the figures of the host emulation, i.e. device powf acts as correctly rounded here; the four multi tables
    p <= 0.992, m <= 0.639, v <= 0.326; the cross-check bit-equal in all five modes; FusedAdam over views, three steps
    against the summed bands, p 0.199, m 0.616, v 0.410."""
    case = R.BIG_CASE
    assert R.pw_geometry(case.sizes[0])["passes"] == 2
    keep = []
    try:
        data = [R.draw(case.sizes[0], case.seed, case.mode["S"], device=dev)]
        s = State(case, data, dev)
        launch_pw(s, 0, block(case, dev, keep))
        s.check()
    finally:
        s = data = None
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 5: refused arguments launch nothing
def test_refused_arguments_launch_nothing(dev):
    """p, g, m or v 4, 8 or 12 bytes off a 16-byte boundary and a shadow 2, 4 or 6 bytes off an 8-byte one: -1, the message,
    and not one word of any buffer written.  The first refused call carries found_inf = 1, under which no build's kernel
    touches a tensor; only a build that refuses that call is given the others."""
    L = P("_lib")
    lib = L.lib()
    can = Canaries(dev)
    n = 64
    bufs = [can.alloc((n + 8,), torch.float32, what) for what in "pgmv"]
    sh = can.alloc((n + 8,), torch.bfloat16, "shadow")
    step = torch.ones(1, dtype=torch.int32, device=dev)
    set_flag = torch.ones(1, device=dev)
    for b in bufs:
        assert b.data_ptr() % 16 == 0
    blocked = adam_args(step, found_inf=set_flag)
    rc = lib.dsr_pw_adam(ptr(bufs[0], 4), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), n, None, blocked, stream())
    assert rc == -1 and b"16-byte aligned" in lib.dsr_last_error()
    scale = torch.full((1,), 4.0, device=dev)
    hyper = torch.tensor([1e-3, 1.0], device=dev)
    for blk in (adam_args(step), adam_args(step, loss_scale=scale, found_inf=torch.zeros(1, device=dev)), adam_args(step, hyper=hyper)):
        for off in (4, 8, 12):
            for slot in range(4):
                ops = [ptr(b, off if i == slot else 0) for i, b in enumerate(bufs)]
                for shadow in (None, ptr(sh)):
                    assert lib.dsr_pw_adam(*ops, n, shadow, blk, stream()) == -1, (off, slot)
                    assert b"16-byte aligned" in lib.dsr_last_error()
        for off in (2, 4, 6):
            assert lib.dsr_pw_adam(*[ptr(b) for b in bufs], n, ptr(sh, off), blk, stream()) == -1, off
            assert b"8-byte aligned" in lib.dsr_last_error()
    can.check()
    assert all(can.untouched(b) for b in bufs) and can.untouched(sh)
    assert step.item() == 1


# ----------------------------------------------------------------------------- 6: FusedAdam over views off a 16-byte boundary
def test_fused_adam_updates_views_off_a_16_byte_boundary(dev, monkeypatch):
    """Parameters and gradients that are views 4, 8 and 12 bytes off a 16-byte boundary, three of them above (a lowered)
    MULTI_MAX: three steps against three chained adam_step()s, elementwise, the per-step bands summed.  No dsr_pw_adam call
    carries a misaligned pointer: a skewed parameter takes the multi-tensor launch whatever its size, a skewed gradient bound
    for the per-tensor launch is copied; aligned tensors keep the per-tensor launch on their own storage."""
    O, L, F = P("optim"), P("_lib"), P("functional")
    lib = L.lib()
    #        n     p off  g off
    spec = [(4099, 4, 0), (257, 0, 8), (8193, 12, 4), (6001, 0, 12), (8195, 0, 0), (1023, 8, 12), (7000, 8, 0)]
    big = [i for i, (n, po, _) in enumerate(spec) if n > 5000 and po == 0]           # per-tensor launches: 3 and 4
    lr, b1, b2, eps = (R.F32(x) for x in R.SETS[0])
    steps = [[R.draw(n, 500 + 10 * it + i, 1.0) for i, (n, _, _) in enumerate(spec)] for it in range(3)]
    pa = R.Arena([d[0] for d in steps[0]], [s[1] for s in spec], dev)
    ga = R.Arena([d[1] for d in steps[0]], [s[2] for s in spec], dev)
    params = [v.requires_grad_(True) for v in pa.views]
    for p, g in zip(params, ga.views):
        p.grad = g
    opt = O.FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps)
    opt.MULTI_MAX = 5000
    calls = []
    real = lib.dsr_pw_adam

    def spy(p, g, m, v, n, sh, args, st):
        calls.append((p.value, g.value, m.value, v.value, n))
        return real(p, g, m, v, n, sh, args, st)

    monkeypatch.setattr(lib, "dsr_pw_adam", spy)
    ref = [(d[0].double(), torch.zeros(d[0].numel(), dtype=torch.float64), torch.zeros(d[0].numel(), dtype=torch.float64))
           for d in steps[0]]
    band = [[torch.zeros(d[0].numel(), dtype=torch.float64) for _ in range(3)] for d in steps[0]]
    names = []
    for it in range(3):
        for i, d in enumerate(steps[it]):
            ga.views[i].copy_(d[1])
        L.LAUNCH_LOG = []
        try:
            opt.step()
            names.append([n for n, _, _ in L.LAUNCH_LOG])
        finally:
            L.LAUNCH_LOG = None
        for i, d in enumerate(steps[it]):
            out = R.adam_step(ref[i][0], d[1], ref[i][1], ref[i][2], it + 1, lr, b1, b2, eps, 1.0, bands=True)
            ref[i] = out[:3]
            for j in range(3):
                band[i][j] += out[3 + j]
    torch.cuda.synchronize()
    assert names == [["dsr_pw_incr"] + ["dsr_pw_adam"] * len(big) + ["dsr_pw_adam_multi"]] * 3, names
    assert len(calls) == 3 * len(big)
    for k, (p, g, m, v, n) in enumerate(calls):
        i = big[k % len(big)]
        assert p % 16 == g % 16 == m % 16 == v % 16 == 0, (k, p % 16, g % 16)
        assert p == params[i].data_ptr() and n == spec[i][0]
        assert (g == ga.views[i].data_ptr()) == (spec[i][2] == 0)                    # an aligned gradient is not copied
    worst = [0.0, 0.0, 0.0]
    for i, prm in enumerate(params):
        got = (prm.detach().cpu(), opt.m[i].cpu(), opt.v[i].cpu())
        for j in range(3):
            err = (got[j].double() - ref[i][j]).abs()
            r = torch.where(err == 0, err, err / band[i][j])
            worst[j] = max(worst[j], float(r.max()))
            assert float(r.max()) <= 1.0, (i, spec[i], "pmv"[j], float(r.max()), int((r > 1).sum()))
    print(f"FusedAdam over views, 3 steps: worst |delta|/summed band  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert pa.guards_intact() and ga.guards_intact()
    for i, d in enumerate(steps[2]):                                                 # the gradients were read, never written
        assert bool((ga.views[i].cpu().view(torch.int32) == d[1].view(torch.int32)).all())
    # a skewed parameter with a bf16 shadow has no launch that could serve it: refused by name, nothing in the product makes one
    import weakref
    w = params[0]
    shadow = torch.zeros(w.shape, dtype=torch.bfloat16, device=dev)
    monkeypatch.setitem(F._shadow_cache, (id(w), torch.bfloat16, tuple(w.shape)), (F._version(w), shadow, weakref.ref(w)))
    before = len(calls)
    with pytest.raises(ValueError, match="parameter 0 .*4 bytes off a 16-byte boundary.*shadow"):
        opt.step()
    assert len(calls) == before
