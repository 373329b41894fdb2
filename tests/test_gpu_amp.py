"""GPU: the device-side dynamic loss scaler (optim.DynamicLossScaler, the dsr_amp_* kernels of csrc/pointwise.hip and the Adam
entry points with loss_scale / found_inf in their dsr_adam_args).

The yardstick is torch's own scaler on the device: torch.amp.GradScaler beside torch.optim.Adam and the two ops under it
(torch._amp_foreach_non_finite_check_and_unscale_, torch._amp_update_scale_).  Scale, growth counter, overflow flag and the
set of skipped steps must equal torch's exactly.  Every factor is a power of two, so un-scaling is exact and a run under the
scaler must equal, bit for bit, the run under the static scale it sits at: the DIP tests assert equality, not closeness.
Inf and NaN are ordinary float values in buffers here; nothing in this file can fault the device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from adam_args import adam_args
from oracle import dip, downsampler, filler, gan

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
FLT_MAX = 3.4028234663852886e38
CHUNK = 8192              # DSR_AMP_CHUNK: elements of a tensor's 16-byte aligned body that one block of the check reads
SIZES = (1, 7, 4096, 4097, (1 << 20) + 3)


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


def table(tensors):
    k = len(tensors)
    return (k, (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in tensors]),
            (C.c_size_t * k)(*[0 if t is None else t.numel() for t in tensors]))


def amp_check(tensors, found):
    L = P("_lib")
    L.check(L.lib().dsr_amp_check(*table(tensors), ptr(found), stream()))


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ----------------------------------------------------------------------------- 5: the check kernel
def _check_tables(dev):
    """Tensors of SIZES elements, each once 16-byte aligned and once as a view 4 bytes off a 16-byte boundary, then a NULL entry
    and 64 five-element tensors (so the table takes two launches).  Clean data: N(0,1) with FLT_MAX, -FLT_MAX, denormals and
    zeros planted."""
    g = torch.Generator(device="cpu").manual_seed(11)
    special = torch.tensor([FLT_MAX, -FLT_MAX, 1e-40, -1e-45, 0.0, -0.0])
    probes = []
    for off in (0, 1):
        for n in SIZES:
            buf = torch.randn(n + off, generator=g)
            idx = torch.randint(0, n + off, (min(n, 64),), generator=g)
            buf[idx] = special[torch.arange(len(idx)) % len(special)]
            t = buf.to(dev)[off:]
            assert t.numel() == n and t.data_ptr() % 16 == 4 * off
            probes.append(t)
    filler_ = [torch.randn(5, generator=g).to(dev) for _ in range(64)]
    return probes, probes[:5] + [None] + filler_ + probes[5:]


def _torch_found(tensors, dev):
    found = torch.zeros(1, device=dev)
    torch._amp_foreach_non_finite_check_and_unscale_([t.clone() for t in tensors if t is not None], found,
                                                     torch.ones(1, device=dev))
    return found.item()


def test_check_kernel_equals_torchs_non_finite_check(dev):
    probes, tensors = _check_tables(dev)
    assert len(tensors) > 64 and any(t is None for t in tensors)
    found = torch.zeros(1, device=dev)
    amp_check(tensors, found)
    assert found.item() == 0.0 == _torch_found(tensors, dev)          # FLT_MAX, denormals and zeros are finite
    cases = 0
    for t in probes:
        n = t.numel()
        head = min(n, ((16 - t.data_ptr() % 16) % 16) // 4)
        places = {0, n - 1, head - 1, head, head + CHUNK - 1, head + CHUNK, n - 2, (n - head) // 4 * 4 + head - 1}
        for i in sorted(p for p in places if 0 <= p < n):
            for bad in (float("inf"), float("-inf"), float("nan")):
                keep = t[i].clone()
                t[i] = bad
                found.zero_()
                amp_check(tensors, found)
                got, want = found.item(), _torch_found(tensors, dev)
                t[i] = keep
                assert got == want == 1.0, (n, t.data_ptr() % 16, i, bad, got, want)
                cases += 1
    print(f"\ncheck kernel: {cases} planted values found, as torch finds them")
    found.zero_()
    amp_check(tensors, found)
    assert found.item() == 0.0                                        # every planted value was taken out again
    found.fill_(1.0)
    amp_check(tensors, found)
    assert found.item() == 1.0                                        # the check never clears the flag
    only_null = [None, None]
    found.zero_()
    amp_check(only_null, found)
    assert found.item() == 0.0


# ----------------------------------------------------------------------------- 6: predicated Adam
ADAM = (1e-2, 0.9, 0.999, 1e-8)


def _adam_state(dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.randn(n, generator=g).to(dev) for n in SIZES]
    return dict(p=ps, m=[torch.zeros_like(p) for p in ps], v=[torch.zeros_like(p) for p in ps],
                sh=[torch.zeros(p.numel(), dtype=torch.bfloat16, device=dev) for p in ps],
                step=torch.zeros(1, dtype=torch.int32, device=dev))


def _grads(dev, seed, scale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(n, generator=g) * scale).to(dev) for n in SIZES]


def _snapshot(s):
    return [bits(t) for k in ("p", "m", "v", "sh") for t in s[k]] + [bits(s["step"])]


def _equal(a, b):
    return all(bool((x == y).all()) for x, y in zip(a, b))


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("S", [1.0, 1024.0, 65536.0])
def test_predicated_adam_bit_for_bit(dev, S, multi):
    """found_inf = 0: p, m, v, the bf16 shadow and the step counter after the Adam launches in the scaler's mode of dsr_adam_args
    (loss_scale, found_inf; dsr_pw_incr with found_inf) equal those after the plain mode with grad_scale = 1/S (dsr_pw_incr
    without), three steps in a row.  found_inf = 1: nothing moves, NaN gradients included.  (The multi-tensor launch has no
    shadow; its shadow buffers stay zero on both sides.)"""
    L = P("_lib")
    lib, st = L.lib(), stream()
    a, b = _adam_state(dev, 3), _adam_state(dev, 3)
    scale = torch.full((1,), S, device=dev)
    found = torch.zeros(1, device=dev)
    plain = adam_args(a["step"], *ADAM, grad_scale=1.0 / S)
    amp = adam_args(b["step"], *ADAM, loss_scale=scale, found_inf=found)

    def adam(s, gs, args):
        if multi:
            k, pp, ns = table(s["p"])
            L.check(lib.dsr_pw_adam_multi(k, pp, table(gs)[1], table(s["m"])[1], table(s["v"])[1], ns, args, st))
        else:
            for i, g in enumerate(gs):
                L.check(lib.dsr_pw_adam(ptr(s["p"][i]), ptr(g), ptr(s["m"][i]), ptr(s["v"][i]), g.numel(), ptr(s["sh"][i]), args, st))

    for it in range(3):
        gs = _grads(dev, 100 + it, S)
        L.check(lib.dsr_pw_incr(ptr(a["step"]), None, st))
        L.check(lib.dsr_pw_incr(ptr(b["step"]), ptr(found), st))
        adam(a, gs, plain)
        adam(b, gs, amp)
        assert _equal(_snapshot(a), _snapshot(b)), (S, multi, it)
    assert b["step"].item() == 3 and found.item() == 0.0
    before = _snapshot(b)
    found.fill_(1.0)
    for poison in (None, float("nan"), float("inf")):
        gs = _grads(dev, 200, S)
        if poison is not None:
            for g in gs:
                g[g.numel() // 2] = poison
        L.check(lib.dsr_pw_incr(ptr(b["step"]), ptr(found), st))
        adam(b, gs, amp)
        assert _equal(before, _snapshot(b)), (S, multi, poison)
    assert found.item() == 1.0 and scale.item() == S


# ----------------------------------------------------------------------------- 7: the update rule
def _drive(dev, overflow_at, steps, **kw):
    """One-element parameter whose gradient is Inf at the planted steps, under both scalers.  Returns per step
    (our scale, our tracker, our found_inf after update, torch's scale, torch's tracker) and our counts()."""
    O = P("optim")
    ours = O.DynamicLossScaler(**kw)
    theirs = torch.amp.GradScaler("cuda", **kw)
    po = torch.ones(1, device=dev, requires_grad=True)
    pt = torch.ones(1, device=dev, requires_grad=True)
    oo, ot = O.FusedAdam([po], lr=1e-3), torch.optim.Adam([pt], lr=1e-3)
    rows = []
    for it in range(steps):
        g = float("inf") if it in overflow_at else 1.0
        ours.scale(torch.zeros((), device=dev))
        theirs.scale(torch.zeros((), device=dev))
        po.grad = torch.full((1,), g, device=dev)
        pt.grad = torch.full((1,), g, device=dev)
        ours.step(oo)
        ours.update()
        theirs.step(ot)
        theirs.update()
        rows.append((ours._scale.item(), ours._growth_tracker.item(), ours._found_inf.item(), theirs._scale.item(),
                     theirs._growth_tracker.item()))
    return rows, ours.counts()


def test_update_rule_equals_grad_scaler(dev):
    planted = {0, 1, 5, 6, 7, 12, 20, 21, 33, 39}
    rows, counts = _drive(dev, planted, 40, init_scale=2.0 ** 16, growth_interval=3)
    for it, (s, t, f, ts, tt) in enumerate(rows):
        assert (s, t) == (ts, tt), (it, rows[it])
        assert f == 0.0, it
    assert counts == (40 - len(planted), len(planted))
    assert len({r[0] for r in rows}) > 3                       # the sequence both shrinks and grows
    # growth from 2**126: 2**127 is finite and taken, 2**128 is not and is refused, as torch refuses it
    rows, counts = _drive(dev, set(), 4, init_scale=2.0 ** 126, growth_interval=1)
    assert [r[0] for r in rows] == [r[3] for r in rows] == [2.0 ** 127] * 4
    assert [r[1] for r in rows] == [r[4] for r in rows] and counts == (4, 0)


# ----------------------------------------------------------------------------- 8: the whole optimizer
def _quadratic(dev, n=5000, seed=0):
    rng = np.random.default_rng(seed)
    e = torch.tensor(np.logspace(0, 3, n), dtype=torch.float32, device=dev)
    b = torch.tensor(rng.standard_normal(n), dtype=torch.float32, device=dev)
    return (lambda x: 0.5 * (e * x * x).sum() - (b * x).sum()), rng.standard_normal(n)


def _params(x0, dev, splits=(7, 1000, 3993)):
    ps, o = [], 0
    for s in splits:
        ps.append(torch.tensor(x0[o:o + s], dtype=torch.float32, device=dev).requires_grad_(True))
        o += s
    unused = torch.full((3,), 0.5, device=dev, requires_grad=True)          # its gradient stays None
    return ps, ps[:1] + [unused] + ps[1:]


def _run_scaled(dev, kind, steps, inject, scaler=None, start=None):
    """kind: 'fused' (FusedAdam + DynamicLossScaler), 'torch' (torch.optim.Adam + GradScaler), 'plain-fused' / 'plain-torch'
    (no scaler, no injection).  Returns parameters, optimizer, scaler, per-step (scale, taken)."""
    O = P("optim")
    f, x0 = _quadratic(dev)
    ps, allp = start if start is not None else _params(x0, dev)
    kw = dict(init_scale=2.0 ** 16, growth_interval=5)
    if kind == "fused":
        opt, sc = O.FusedAdam(allp, lr=1e-2), scaler or O.DynamicLossScaler(**kw)
    elif kind == "torch":
        opt, sc = torch.optim.Adam(allp, lr=1e-2), scaler or torch.amp.GradScaler("cuda", **kw)
    else:
        opt, sc = (O.FusedAdam if kind == "plain-fused" else torch.optim.Adam)(allp, lr=1e-2), None
    rows = []
    for it in range(steps):
        opt.zero_grad()
        loss = f(torch.cat(ps))
        if sc is None:
            loss.backward()
            opt.step()
            continue
        before = [bits(p) for p in ps]
        sc.scale(loss).backward()
        if it in inject:
            ps[1].grad[5] = float("inf")
        sc.step(opt)
        sc.update()
        taken = any(bool((bits(p) != q).any()) for p, q in zip(ps, before))
        rows.append((float(sc._scale.item()), taken))
    return ps, opt, sc, rows


def rel(a, b):
    a, b = torch.cat([t.detach().double().cpu() for t in a]), torch.cat([t.detach().double().cpu() for t in b])
    return float((a - b).norm() / b.norm())


def test_whole_optimizer_against_torch_adam_and_grad_scaler(dev):
    inject = {3, 4, 11}
    pf, of, sf, rf = _run_scaled(dev, "fused", 30, inject)
    pt, ot, st_, rt = _run_scaled(dev, "torch", 30, inject)
    assert rf == rt                                                      # (a) same scale after every step, same skipped steps
    assert [i for i, r in enumerate(rf) if not r[1]] == sorted(inject)
    assert sf.counts() == (27, 3) and of.step_t.item() == 27
    pp, op, _, _ = _run_scaled(dev, "plain-fused", 27, set())            # (b) the 27 taken steps without any scale
    for a, b in zip(pf, pp):
        assert same(a, b)
    for a, b in zip(of.m + of.v, op.m + op.v):
        assert same(a, b)
    pq, _, _, _ = _run_scaled(dev, "plain-torch", 27, set())             # (c) the floor: FusedAdam against torch.optim.Adam
    floor, err = rel(pp, pq), rel(pf, pt)
    print(f"\nquadratic, 27 taken steps: scaled fused vs scaled torch {err:.3e}; unscaled fused vs torch floor {floor:.3e}")
    assert err <= 2 * floor
    # a checkpoint moves between the two scalers, both ways, and the continued runs still agree
    O = P("optim")
    sf2, st2 = O.DynamicLossScaler(), torch.amp.GradScaler("cuda")
    sf2.load_state_dict(st_.state_dict())
    st2.load_state_dict(sf.state_dict())
    assert sf2.state_dict() == st_.state_dict() == sf.state_dict()
    more = {2}
    _, _, sf3, rf2 = _run_scaled(dev, "fused", 8, more, scaler=sf2)
    _, _, st3, rt2 = _run_scaled(dev, "torch", 8, more, scaler=st2)
    assert rf2 == rt2 and sf3.state_dict() == st3.state_dict()
    assert len({r[0] for r in rf2}) > 1


# ----------------------------------------------------------------------------- 9-13: DIP at config-1 shapes
def _dip(dev, loss_scale):
    """_dip_run of tests/test_gpu_baseline_configs.py: HR 128x128, x2, default 5-scale fp16 skip net, Adam 0.01, sigma 0.05."""
    M, D, steps = P("models.DIP"), P("utils.downsampler"), P("steps")
    P("functional").clear_pack_cache()
    sd = filler.fill_state_dict(gan.template(dip.skip_shapes(dip.SkipConfig(input_depth=32))))
    net = M.get_net(32, "skip", "reflection", upsample_mode="bilinear")
    net.load_state_dict(sd)
    net.to(dev).train()
    assert net.compute_dtype == torch.float16
    down = D.Downsampler(3, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
    hr = filler.tensor("in:c1_hr", (1, 3, 128, 128), 0.5, 0.5)
    lr_img = downsampler.downsampler_forward(hr, 2, "lanczos2", phase=0.5, preserve_size=True).to(dev)
    zin = filler.tensor("in:c1_z", (1, 32, 128, 128), 0.05, 0.05).to(dev)
    return steps.DipRunner(net, down, zin, lr_img, 0.01, 0.05, loss_scale=loss_scale), down, zin, lr_img


def _noise(it, dev):
    return filler.tensor(f"in:c1_noise{it}", (1, 32, 128, 128), 1.7).to(dev)


def _opt_state(run):
    return [bits(p) for p in run.net.parameters()] + [bits(t) for t in run.opt.m + run.opt.v] + [bits(run.opt.step_t)]


def _bn_stats(run):
    return [bits(b) for n, b in run.net.named_buffers() if n.endswith(("running_mean", "running_var"))]


def _static_1024(dev, iters=10):
    run = _dip(dev, 1024.0)[0]
    trace = []
    for it in range(iters):
        loss, out = run.step(_noise(it, dev))
        trace.append((bits(loss), bits(out)))
    return run, trace


def test_dip_scaler_at_rest_equals_the_static_path(dev):
    O = P("optim")
    ref, trace = _static_1024(dev)
    run = _dip(dev, O.DynamicLossScaler(init_scale=1024.0, growth_interval=10 ** 9))[0]
    assert run.scaler is not None and run.opt.grad_scale == 1.0
    for it in range(10):
        loss, out = run.step(_noise(it, dev))
        assert bool((bits(loss) == trace[it][0]).all()) and bool((bits(out) == trace[it][1]).all()), it
    assert _equal(_opt_state(run), _opt_state(ref))
    assert run.scaler.counts() == (10, 0) and run.scaler.get_scale() == 1024.0


_dip_start = []


def dip_start(dev):
    """The initial scale of the 'at work' runs: 2**24, raised by 2**4 at a time until the first iteration overflows fp16 (where
    that happens had not been measured when this was written; a start whose first step is taken would test nothing)."""
    if not _dip_start:
        O = P("optim")
        for e in range(24, 64, 4):
            sc = O.DynamicLossScaler(init_scale=2.0 ** e, growth_interval=10 ** 9)
            _dip(dev, sc)[0].step(_noise(0, dev))
            if sc.counts() == (0, 1):
                _dip_start.append(2.0 ** e)
                break
        print(f"\nDIP config 1: the first iteration overflows from an initial scale of 2**{e}")
    assert _dip_start, "no initial scale up to 2**60 made the first iteration overflow"
    return _dip_start[0]


def test_dip_scaler_at_work_skips_then_equals_the_static_scale_it_finds(dev):
    O = P("optim")
    DIP_START = dip_start(dev)
    sc = O.DynamicLossScaler(init_scale=DIP_START, growth_interval=10 ** 9)
    run = _dip(dev, sc)[0]
    taken_its, prev = [], (0, 0)
    for it in range(10):
        before, stats = _opt_state(run), _bn_stats(run)
        run.step(_noise(it, dev))
        now = sc.counts()
        if now[1] > prev[1]:                                        # skipped: nothing of the optimizer moves ...
            assert not taken_its, "a skipped step after a taken one: the scale only falls here"
            assert _equal(before, _opt_state(run)), it
            assert not _equal(stats, _bn_stats(run)), it            # ... while BatchNorm's running statistics do, as in torch
        else:
            taken_its.append(it)
        prev = now
    taken, skipped = sc.counts()
    s_star = sc.get_scale()
    print(f"\nDIP config 1 from 2**{int(np.log2(DIP_START))}: {skipped} steps skipped, first step taken at S* = 2**{int(np.log2(s_star))}")
    assert skipped >= 1 and taken == len(taken_its) == 10 - skipped >= 1
    assert DIP_START / 2 ** skipped == s_star
    assert run.opt.step_t.item() == taken
    ref = _dip(dev, s_star)[0]
    for it in taken_its:
        ref.step(_noise(it, dev))
    assert _equal(_opt_state(run), _opt_state(ref))
    assert all(bool(torch.isfinite(p).all()) for p in run.net.parameters())


def test_dip_scaler_grows_from_one(dev):
    O = P("optim")
    sc = O.DynamicLossScaler(init_scale=1.0, growth_interval=2)
    run = _dip(dev, sc)[0]
    scale = torch.ones(1, device=dev)
    tracker = torch.zeros(1, dtype=torch.int32, device=dev)
    losses, prev = [], (0, 0)
    for it in range(40):
        loss, _ = run.step(_noise(it, dev))
        losses.append(loss.item())
        now = sc.counts()
        found = torch.full((1,), float(now[1] > prev[1]), device=dev)
        prev = now
        torch._amp_update_scale_(scale, tracker, found, 2.0, 0.5, 2)
        assert sc._scale.item() == scale.item() and sc._growth_tracker.item() == tracker.item(), it
        for t in list(run.net.parameters()) + run.opt.m + run.opt.v:
            assert bool(torch.isfinite(t).all()), it
    print(f"\nDIP config 1 from scale 1, growth every 2 clean steps: scale after 40 iterations 2**{int(np.log2(sc.get_scale()))}, "
          f"(taken, skipped) = {sc.counts()}, loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert sc.get_scale() > 1.0
    assert losses[-1] < losses[0]


def test_dip_dynamic_step_replays_in_a_graph(dev):
    """GraphedStep over the dynamic step (capture fails if anything reads the device from the host): replays equal eager steps
    bit for bit across the skipped-then-taken transition, and a skipped iteration launches what a taken one launches."""
    O, S, L = P("optim"), P("steps"), P("_lib")
    start = dip_start(dev) * 4
    iters = 12

    def seq(i):                        # GraphedStep's single warm-up step runs on noise 0, then the replays follow
        return _noise(max(i - 1, 0), dev)

    eager_sc = O.DynamicLossScaler(init_scale=start, growth_interval=10 ** 9)
    eager = _dip(dev, eager_sc)[0]
    trace, names, skipped_flags, prev = [], [], [], 0
    for i in range(iters):
        L.LAUNCH_LOG = []
        try:
            loss, out = eager.step(seq(i))
            names.append([n for n, _, _ in L.LAUNCH_LOG])
        finally:
            L.LAUNCH_LOG = None
        trace.append((bits(loss), bits(out)))
        now = eager_sc.counts()[1]
        skipped_flags.append(now > prev)
        prev = now
    assert skipped_flags[1] and not skipped_flags[-1], skipped_flags     # the transition happens among the replays
    first_taken = skipped_flags.index(False)
    assert names[1] == names[first_taken] == names[-1]
    assert "dsr_amp_check" in names[1] and "dsr_amp_update" in names[1] and "dsr_pw_adam_multi" in names[1]
    # the counter is the predicated one: one launch per step, and it stood still through the skipped iterations
    assert all(n.count("dsr_pw_incr") == 1 for n in names)
    taken = eager_sc.counts()[0]
    assert eager.opt.step_t.item() == taken == iters - sum(skipped_flags) < iters

    sc = O.DynamicLossScaler(init_scale=start, growth_interval=10 ** 9)
    run = _dip(dev, sc)[0]
    noise = seq(0).clone()
    graphed = S.GraphedStep(lambda: run.step(noise), warmup=1)
    for i in range(1, iters):
        noise.copy_(seq(i))
        loss, out = graphed()
        assert bool((bits(loss) == trace[i][0]).all()) and bool((bits(out) == trace[i][1]).all()), i
    assert _equal(_opt_state(run), _opt_state(eager))
    assert sc.counts() == eager_sc.counts() and sc.get_scale() == eager_sc.get_scale()


def test_dropin_optimize_with_dynamic_loss_scale(dev):
    """utils.DIP.optimize('adam', ..., loss_scale=...) around a closure written as the reference's DIP.py:47-95 writes it: the
    loss is never scaled by the caller, the scale enters at the net output's backward -- and the parameters equal those of
    DipRunner under static 1024 bit for bit.  Without the keyword the gradients are unscaled, as before: other parameters."""
    O, D, F = P("optim"), P("utils.DIP"), P("functional")
    ref, _ = _static_1024(dev)
    want = [bits(p) for p in ref.net.parameters()]

    def dropin(**kw):
        run, down, zin, lr_img = _dip(dev, 1.0)
        net, it = run.net, [0]

        def closure():
            net_input = zin + _noise(it[0], dev) * 0.05
            out_hr = net(net_input)
            out_lr = down(out_hr)
            total_loss = F.mse_loss(out_lr, lr_img)
            total_loss.backward()
            it[0] += 1
            return total_loss

        D.optimize("adam", D.get_params("net", net, zin), closure, 0.01, 10, **kw)
        assert it[0] == 10 and F._ambient_scale is None
        return [bits(p) for p in net.parameters()]

    sc = O.DynamicLossScaler(init_scale=1024.0, growth_interval=10 ** 9)
    got = dropin(loss_scale=sc)
    assert sc.counts() == (10, 0)
    assert _equal(got, want)
    assert not _equal(dropin(), want)


# ----------------------------------------------------------------------------- 14: generator step, refusals
def test_gen_l1_step_with_a_scaler_at_rest_and_refusals(dev):
    O, S = P("optim"), P("steps")
    gen = P("models.GAN.generator")
    lr = filler.tensor("in:traj_lr", (4, 3, 24, 24), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:traj_hr", (4, 3, 96, 96)).to(dev)

    def run(scaler):
        P("functional").clear_pack_cache()
        g = gen.Generator(4, 2)
        g.load_state_dict(filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2))))
        g.to(dev).train()
        for m in g.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = torch.float16
        opt = O.FusedAdam(g.parameters(), lr=1e-4)
        out = []
        for _ in range(4):
            loss, fake = S.gen_l1_step(g, opt, lr, hr) if scaler is None else S.gen_l1_step(g, opt, lr, hr, scaler=scaler)
            out += [bits(loss), bits(fake)]
        return out + [bits(p) for p in g.parameters()] + [bits(t) for t in opt.m + opt.v] + [bits(opt.step_t)]

    sc = O.DynamicLossScaler(init_scale=1.0, growth_interval=10 ** 9)
    assert _equal(run(None), run(sc))
    assert sc.counts() == (4, 0) and sc.get_scale() == 1.0
    p = torch.ones(8, device=dev, requires_grad=True)
    p.grad = torch.ones(8, device=dev)
    with pytest.raises(ValueError, match="dense head"):
        O.FusedAdam([p], fuse_dense_head=True).step(scaler=sc)
    with pytest.raises(ValueError, match="twice"):
        O.FusedAdam([p], grad_scale=0.5).step(scaler=sc)
    with pytest.raises(ValueError, match="twice"):
        sc.step(O.FusedAdam([p], grad_scale=0.5))
    assert bool((p == 1).all())
    off = O.DynamicLossScaler(enabled=False)
    opt = O.FusedAdam([p], lr=0.5)
    off.step(opt)                                                       # a plain optimizer.step(), as in torch
    off.update()
    assert opt.step_t.item() == 1 and bool((p < 1).all())
