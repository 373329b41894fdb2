"""GPU: optim.WeightEMA and the dsr_ema_* kernels of csrc/ema.hip against tests/ema_ref.py (float64, exact rational weights).

Tolerance (derived, not measured): one update rounds the decay (or the warm-up quotient), 1 - d, p - s, the product and the
sum in fp32 -- at most about eight roundings of 2^-24 relative on quantities bounded by 2 M, M the largest |p| or |shadow|
of the tensor seen so far -- and the recurrence is a contraction, so errors add and never grow: after K updates
|shadow - ref| <= K * 2^-21 * M elementwise.  Exact copies (the first update of the torch mode, `copy`-flagged tensors, swap,
copy_to, restore) are compared bit for bit.  Inf and NaN are ordinary float values in buffers here; nothing in this file can
fault the device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import ema_ref
from oracle import filler, gan

pytestmark = pytest.mark.gpu
PKG = "deep-super-resolution_amd"
GUARD = 0x7FC0BEEF             # a NaN payload no arithmetic here produces
SIZES = (1, 3, 5, 7, 8, 63, 64, 65, 4097, (1 << 20) + 5)


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
    t = t.detach().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).clone()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def bound(K, M):
    return K * 2.0 ** -21 * M


# ----------------------------------------------------------------------------- the tensor set of the kernel tests
def _layout():
    """65 entries: (n, word offset of the shadow from a 16-byte boundary, word offset of the parameter, copy flag, kind)."""
    ents = [(n, 0, 0, 0, "run") for n in SIZES]
    ents.append((8, 0, 0, 0, "empty"))                     # passed with n = 0
    ents.append((16, 0, 0, 0, "null"))                     # passed as two NULL pointers
    ents += [(8200, 1, 1, 0, "run"), (70, 2, 2, 0, "run"), (9, 3, 3, 0, "run")]      # views 4 / 8 / 12 bytes off
    ents += [(5000, 1, 0, 0, "run"), (6, 0, 2, 0, "run")]   # the two sides at different offsets: the 4-byte path, two blocks
    ents += [(33, 0, 0, 1, "run"), (4100, 3, 3, 1, "run")]  # copied whatever the counter says
    i = 0
    while len(ents) < 65:
        ents.append((2 + i % 19, 0, 0, 0, "run"))
        i += 1
    order = [0, 9] + [k for k in range(len(ents)) if k not in (0, 9)]     # the big tensor early: both launches hold many blocks
    return [ents[k] for k in order]


class Arena:
    """One fp32 buffer holding every tensor of a side between 4 guard words before and after it."""

    def __init__(self, ents, side, dev, seed):
        pos, cur = [], 0
        for n, off_a, off_b, _, _ in ents:
            start = cur + 4
            start += (-(start) + (off_a, off_b)[side]) % 4
            pos.append(start)
            cur = start + n + 4
        g = torch.Generator(device="cpu").manual_seed(seed)
        host = torch.randn(cur, generator=g, dtype=torch.float32)
        self.guard = torch.ones(cur, dtype=torch.bool)
        for (n, *_), s in zip(ents, pos):
            self.guard[s:s + n] = False
        host.view(torch.int32)[self.guard] = GUARD
        self.buf = host.to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[s:s + n] for (n, *_), s in zip(ents, pos)]
        for (n, off_a, off_b, _, _), v in zip(ents, self.views):
            assert (v.data_ptr() % 16) // 4 == (off_a, off_b)[side]
        self.guard = self.guard.to(dev)

    def guards_intact(self):
        return bool((self.buf.view(torch.int32)[self.guard] == GUARD).all())


def _tables(ents, a, b):
    k = len(ents)
    pa = [None if e[4] == "null" else v.data_ptr() for e, v in zip(ents, a.views)]
    pb = [None if e[4] == "null" else v.data_ptr() for e, v in zip(ents, b.views)]
    ns = [0 if e[4] == "empty" else e[0] for e in ents]
    return (k, (C.c_void_p * k)(*pa), (C.c_void_p * k)(*pb), (C.c_size_t * k)(*ns),
            (C.c_ubyte * k)(*[e[3] for e in ents]))


def _specials(t):
    """Values a copy must carry bit for bit."""
    vals = torch.tensor([float("nan"), -0.0, float("inf"), 1e-42, -float("inf")], dtype=torch.float32)
    k = min(t.numel(), vals.numel())
    t[:k] = vals[:k].to(t.device)
    if t.numel() > 5:
        t.view(torch.int32)[5] = 0x7FA12345            # a signalling-NaN payload


def _refresh(ents, params, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for e, v in zip(ents, params.views):
        v.copy_(torch.randn(e[0], generator=g, dtype=torch.float32) * 3.0)
        if e[3]:
            _specials(v)


def _as_ref(views):
    with np.errstate(invalid="ignore"):                # (a signalling NaN in a copied tensor)
        return {i: v.detach().cpu().numpy().astype(np.float64) for i, v in enumerate(views)}


@pytest.mark.parametrize("mode", [0, 1])
def test_kernel_against_the_recurrence(dev, mode):
    L = P("_lib")
    lib = L.lib()
    ents = _layout()
    assert len(ents) == 65 and sum(1 for e in ents if e[3]) == 2
    sh, pa = Arena(ents, 0, dev, 1), Arena(ents, 1, dev, 2)
    k, tsh, tpa, ns, flags = _tables(ents, sh, pa)
    n_avg = torch.zeros(1, dtype=torch.int32, device=dev)
    decay, updates = (0.9, 6) if mode == 0 else (0.5, 12)
    active = [i for i, e in enumerate(ents) if e[4] == "run"]
    idle = [i for i, e in enumerate(ents) if e[4] != "run"]
    idle_before = [bits(sh.views[i]) for i in idle]
    ref = ema_ref.EmaRef({i: v for i, v in _as_ref(sh.views).items() if i in active}, buffers=[i for i in active if ents[i][3]],
                         decay=decay, warmup=bool(mode))
    M = {i: float(sh.views[i].abs().max()) for i in active if not ents[i][3]}
    for it in range(updates):
        _refresh(ents, pa, 100 + it, dev)
        before = bits(pa.buf)
        L.check(lib.dsr_ema_update_multi(k, tsh, tpa, ns, flags, decay, mode, ptr(n_avg), None, stream()))
        L.check(lib.dsr_ema_tick(ptr(n_avg), None, stream()))
        torch.cuda.synchronize()
        assert bool((bits(pa.buf) == before).all()), "the parameter side is read only"
        assert sh.guards_intact() and pa.guards_intact(), it
        snap = _as_ref(pa.views)
        ref.update({i: snap[i] for i in active})
        worst = 0.0
        for i in active:
            if ents[i][3] or (mode == 0 and it == 0):
                assert same(sh.views[i], pa.views[i]), (it, i, ents[i])          # an exact copy
                continue
            M[i] = max(M[i], float(pa.views[i].abs().max()), float(sh.views[i].abs().max()))
            err = np.abs(sh.views[i].cpu().numpy().astype(np.float64) - ref.shadow[i]).max()
            worst = max(worst, err / bound(it + 1, M[i]))
            assert err <= bound(it + 1, M[i]), (it, i, ents[i], err, bound(it + 1, M[i]))
        print(f"mode {mode} update {it + 1}: worst error / bound = {worst:.3f}")
    assert n_avg.item() == updates == ref.n_averaged
    for i, b in zip(idle, idle_before):
        assert bool((bits(sh.views[i]) == b).all()), ("skipped entry written", ents[i])
    # an average, not a copy: the last parameters are far from the shadow
    big = next(i for i in active if ents[i][0] == SIZES[-1])
    assert float((sh.views[big] - pa.views[big]).abs().max()) > 1.0


def test_found_inf_freezes_the_average_and_its_counter(dev):
    L = P("_lib")
    lib = L.lib()
    ents = _layout()
    sh, pa = Arena(ents, 0, dev, 3), Arena(ents, 1, dev, 4)
    twin = Arena(ents, 0, dev, 3)                          # the same bits as `sh`, and kept so by every round below
    k, tsh, tpa, ns, flags = _tables(ents, sh, pa)
    _, ttw, _, _, _ = _tables(ents, twin, pa)
    for mode in (0, 1):
        for start in (0, 3):
            _refresh(ents, pa, 200 + 10 * mode + start, dev)
            n_avg = torch.full((1,), start, dtype=torch.int32, device=dev)
            found = torch.ones(1, dtype=torch.float32, device=dev)
            before = bits(sh.buf)
            L.check(lib.dsr_ema_update_multi(k, tsh, tpa, ns, flags, 0.75, mode, ptr(n_avg), ptr(found), stream()))
            L.check(lib.dsr_ema_tick(ptr(n_avg), ptr(found), stream()))
            torch.cuda.synchronize()
            assert bool((bits(sh.buf) == before).all()) and n_avg.item() == start and found.item() == 1.0
            found.zero_()
            L.check(lib.dsr_ema_update_multi(k, tsh, tpa, ns, flags, 0.75, mode, ptr(n_avg), ptr(found), stream()))
            L.check(lib.dsr_ema_tick(ptr(n_avg), ptr(found), stream()))
            # the twin never saw the skipped call (and passes no flag at all)
            n_tw = torch.full((1,), start, dtype=torch.int32, device=dev)
            L.check(lib.dsr_ema_update_multi(k, ttw, tpa, ns, flags, 0.75, mode, ptr(n_tw), None, stream()))
            L.check(lib.dsr_ema_tick(ptr(n_tw), None, stream()))
            torch.cuda.synchronize()
            assert n_avg.item() == n_tw.item() == start + 1
            assert bool((bits(sh.buf) == bits(twin.buf)).all()) and not bool((bits(sh.buf) == before).all())


def test_swap_exchanges_bits(dev):
    L = P("_lib")
    lib = L.lib()
    ents = _layout()
    a, b = Arena(ents, 0, dev, 5), Arena(ents, 1, dev, 6)
    for e, va, vb in zip(ents, a.views, b.views):
        if e[0] >= 7:
            _specials(va)
            _specials(vb[1:])
    k, ta, tb, ns, _ = _tables(ents, a, b)
    a0, b0 = [bits(v) for v in a.views], [bits(v) for v in b.views]
    L.check(lib.dsr_ema_swap_multi(k, ta, tb, ns, stream()))
    torch.cuda.synchronize()
    assert a.guards_intact() and b.guards_intact()
    for i, e in enumerate(ents):
        if e[4] == "run":
            assert bool((bits(a.views[i]) == b0[i]).all()) and bool((bits(b.views[i]) == a0[i]).all()), (i, e)
        else:
            assert bool((bits(a.views[i]) == a0[i]).all()) and bool((bits(b.views[i]) == b0[i]).all()), (i, e)
    L.check(lib.dsr_ema_swap_multi(k, ta, tb, ns, stream()))
    torch.cuda.synchronize()
    assert a.guards_intact() and b.guards_intact()
    assert all(bool((bits(v) == w).all()) for v, w in zip(a.views, a0)) and all(bool((bits(v) == w).all()) for v, w in zip(b.views, b0))


# ----------------------------------------------------------------------------- module level
def _gen(dev, half=False):
    G = P("models.GAN.generator")
    g = G.Generator(factor=2, residual_blocks_count=1)
    g.load_state_dict(filler.fill_state_dict(gan.template(gan.generator_shapes(2, 1))))
    g.to(dev).train()
    if half:
        for m in g.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = torch.float16
    return g


def _batch(dev):
    return (filler.tensor("in:ema_lr", (2, 3, 16, 16), 0.5, 0.5).to(dev), filler.tensor("in:ema_hr", (2, 3, 32, 32)).to(dev))


def _named(module):
    out = dict(module.named_parameters())
    out.update(dict(module.named_buffers()))
    return out


def _clone(module):
    return {k: v.detach().clone() for k, v in _named(module).items()}


def _host(snap):
    return {k: (v.cpu().numpy() if not v.is_floating_point() else v.cpu().numpy().astype(np.float64)) for k, v in snap.items()}


def _buffers(module):
    return [k for k, _ in module.named_buffers()]


def _check_against_ref(ema, module, start, snaps, skipped=(), label=""):
    """The EMA's shadow against ema_ref over the snapshots, within K * 2^-21 * M per tensor; integer tensors exactly."""
    shadows, n = ema_ref.run(_host(start), [_host(s) for s in snaps], _buffers(module), decay=ema.decay, warmup=ema.warmup,
                             use_buffers=ema.use_buffers, skipped=set(skipped))
    want = shadows[-1]
    K = len(snaps)
    got = ema.state_dict()
    assert got["n_averaged"] == n == K - len(set(skipped))
    worst = 0.0
    hosts = [_host(start)] + [_host(s) for s in snaps]
    for name, t in got["shadow"].items():
        if not t.is_floating_point():
            assert np.array_equal(t.cpu().numpy(), want[name]), name
            continue
        M = max(max(float(np.abs(h[name]).max()) for h in hosts), max(float(np.abs(s[name]).max()) for s in shadows))
        err = float(np.abs(t.cpu().numpy().astype(np.float64) - want[name]).max())
        worst = max(worst, err / bound(K, M))
        assert err <= bound(K, M), (label, name, err, bound(K, M))
    print(f"{label}: {K} updates, worst error / bound = {worst:.3f}")
    return want


@pytest.fixture(scope="module")
def trained(dev):
    """Test 8's plain run: 6 eager gen_l1_step(..., ema=ema) calls; shared, and left bitwise as it was by every user."""
    O, S = P("optim"), P("steps")
    g = _gen(dev)
    lr, hr = _batch(dev)
    opt = O.FusedAdam(g.parameters(), lr=1e-3)
    ema = O.WeightEMA(g, decay=0.9)
    start, snaps = _clone(g), []
    for _ in range(6):
        S.gen_l1_step(g, opt, lr, hr, ema=ema)
        snaps.append(_clone(g))
    torch.cuda.synchronize()
    return dict(gen=g, ema=ema, start=start, snaps=snaps, lr=lr, hr=hr, opt=opt)


def test_eager_steps_match_the_recurrence(dev, trained):
    g, ema = trained["gen"], trained["ema"]
    _check_against_ref(ema, g, trained["start"], trained["snaps"], label="eager torch mode")
    live, sd = _named(g), ema.state_dict()["shadow"]
    for name, _ in g.named_buffers():
        assert same(sd[name], live[name]), name                      # use_buffers=False: the buffers follow the model
    w = "conv1.weight"
    gap = float((sd[w] - live[w].detach()).abs().max())
    assert gap > 100 * bound(6, float(live[w].detach().abs().max())), "the average must differ from the weights by far more than the bound"
    assert ema.n_averaged.dtype == torch.int32 and ema.n_averaged.item() == 6 == trained["opt"].step_t.item()


@pytest.mark.parametrize("warmup,use_buffers", [(True, False), (False, True)])
def test_eager_steps_other_policies(dev, warmup, use_buffers):
    O, S = P("optim"), P("steps")
    g = _gen(dev)
    lr, hr = _batch(dev)
    opt = O.FusedAdam(g.parameters(), lr=1e-3)
    ema = O.WeightEMA(g, decay=0.5 if warmup else 0.9, warmup=warmup, use_buffers=use_buffers)
    start, snaps = _clone(g), []
    for _ in range(6):
        S.gen_l1_step(g, opt, lr, hr, ema=ema)
        snaps.append(_clone(g))
    _check_against_ref(ema, g, start, snaps, label=f"eager warmup={warmup} use_buffers={use_buffers}")
    live, sd = _named(g), ema.state_dict()["shadow"]
    ints = [k for k, v in live.items() if not v.is_floating_point()]
    assert ints and all(same(sd[k], live[k]) and int(live[k]) > 0 for k in ints)        # integer buffers: the model's
    if use_buffers:
        assert not same(sd["bn1.running_var"], live["bn1.running_var"])                  # averaged, not copied


def test_skipped_step_under_the_dynamic_scaler(dev):
    O, S, F = P("optim"), P("steps"), P("functional")
    g = _gen(dev, half=True)
    lr, hr = _batch(dev)
    opt = O.FusedAdam(g.parameters(), lr=1e-3)
    sc = O.DynamicLossScaler(init_scale=2.0 ** 7, growth_interval=10 ** 9)
    ema = O.WeightEMA(g, decay=0.9)
    start, snaps = _clone(g), []
    for it in range(6):
        if it != 2:
            S.gen_l1_step(g, opt, lr, hr, scaler=sc, ema=ema)
        else:                                                       # the recipe's own sequence, with an Inf placed in one gradient
            params = [bits(p) for p in g.parameters()]
            shadow = [bits(t) for t in ema._shadow]
            loss = F.l1_loss(g(lr), hr)
            opt.zero_grad()
            with F.batched_wgrad():
                sc.scale(loss).backward()
            next(p for p in g.parameters() if p.grad is not None).grad.view(-1)[1] = float("inf")
            sc.step(opt)
            ema.update(sc)
            sc.update()
            torch.cuda.synchronize()
            assert all(bool((bits(p) == q).all()) for p, q in zip(g.parameters(), params))
            assert all(bool((bits(t) == q).all()) for t, q in zip(ema._shadow, shadow))
            assert ema.n_averaged.item() == 2 == opt.step_t.item()
        snaps.append(_clone(g))
    assert sc.counts() == (5, 1) and sc.get_scale() == 2.0 ** 6
    _check_against_ref(ema, g, start, snaps, skipped={2}, label="fp16 storage, step 3 skipped")
    with pytest.raises(RuntimeError, match=r"scaler\.step\(opt\); ema\.update\(scaler\); scaler\.update\(\)"):
        ema.update(sc)                                              # the flag of the last step is gone: refused on the host


def test_graph_replay(dev):
    O, S = P("optim"), P("steps")
    g = _gen(dev)
    lr, hr = _batch(dev)
    opt = O.FusedAdam(g.parameters(), lr=1e-3)
    ema = O.WeightEMA(g, decay=0.9)
    start, snaps = _clone(g), []

    def fn():
        out = S.gen_l1_step(g, opt, lr, hr, ema=ema)
        if not torch.cuda.is_current_stream_capturing():
            snaps.append(_clone(g))                                  # the eager warm-up steps
        return out

    graphed = S.GraphedStep(fn, warmup=2)                            # capture itself executes nothing
    assert len(snaps) == 2
    for _ in range(5):
        graphed()
        snaps.append(_clone(g))
    torch.cuda.synchronize()
    assert ema.n_averaged.item() == 7 == opt.step_t.item()
    _check_against_ref(ema, g, start, snaps, label="2 eager + 5 replayed")


def _fresh_from(ema, dev):
    G = P("models.GAN.generator")
    f = G.Generator(factor=2, residual_blocks_count=1)
    f.load_state_dict(ema.module_state_dict(), strict=True)
    return f.to(dev).eval()


def test_swapped_weights_reach_the_forward(dev, trained):
    """The stale-cache test: the packed 16-bit weight images and the kept BatchNorm affine maps are warm when the weights are
    exchanged under them."""
    g, ema, x = trained["gen"], trained["ema"], trained["lr"]
    g.eval()
    try:
        with torch.no_grad():
            y0 = g(x).clone()
            y0b = g(x).clone()                                      # (a second call: every cache is in use)
            want = _fresh_from(ema, dev)(x).clone()
        assert same(y0, y0b) and not same(y0, want)
        before = {k: bits(v) for k, v in _named(g).items()}
        averaged = {k: bits(v) for k, v in ema.state_dict()["shadow"].items()}
        with ema.average_parameters():
            with torch.no_grad():
                y1 = g(x).clone()
            assert all(bool((bits(v) == averaged[k]).all()) for k, v in _named(g).items())
        assert same(y1, want)
        with torch.no_grad():
            y2 = g(x).clone()
        assert same(y2, y0)
        assert all(bool((bits(v) == before[k]).all()) for k, v in _named(g).items())
        assert all(bool((bits(v) == averaged[k]).all()) for k, v in ema.state_dict()["shadow"].items())
        # the same through copy_to() / restore()
        ema.copy_to()
        with torch.no_grad():
            y3 = g(x).clone()
        ema.restore()
        with torch.no_grad():
            y4 = g(x).clone()
        assert same(y3, want) and same(y4, y0)
        assert all(bool((bits(v) == before[k]).all()) for k, v in _named(g).items())
        with pytest.raises(RuntimeError, match="copy_to"):
            ema.restore()
        # ... and into another live module whose caches are warm
        other = _gen(dev).eval()
        with torch.no_grad():
            assert not same(other(x), want)
            ema.copy_to(other)
            assert same(other(x), want)
        # an exception inside the block still swaps back
        with pytest.raises(KeyError):
            with ema.average_parameters():
                raise KeyError("boom")
        assert all(bool((bits(v) == before[k]).all()) for k, v in _named(g).items())
    finally:
        g.train()


def test_evaluate_generator_scores_the_average(dev, trained):
    E = P("evaluate")
    g, ema = trained["gen"], trained["ema"]
    pairs = [(filler.tensor(f"in:ema_ev_lr{i}", (1, 3, 16, 16), 0.5, 0.5).to(dev),
              filler.tensor(f"in:ema_ev_hr{i}", (1, 3, 32, 32), 0.5, 0.5).to(dev), f"img{i}") for i in range(2)]
    before = {k: bits(v) for k, v in _named(g).items()}
    was_training = g.training
    try:
        want = E.evaluate_generator(_fresh_from(ema, dev), pairs)
        own = E.evaluate_generator(g, pairs)
        got = E.evaluate_generator(g, pairs, ema=ema)
        assert got == want and got != own
        assert all(bool((bits(v) == before[k]).all()) for k, v in _named(g).items())
        bad = pairs[:1] + [(pairs[1][0], torch.zeros(1, 3, 40, 40, device=dev), "odd")]
        with pytest.raises(RuntimeError, match="shape"):
            E.evaluate_generator(g, bad, ema=ema)
        assert all(bool((bits(v) == before[k]).all()) for k, v in _named(g).items())
        assert E.evaluate_generator(g, pairs) == own
    finally:
        g.train(was_training)


def test_gan_step_with_ema(dev):
    Dm, GANu, O, S = P("models.GAN.discriminator"), P("utils.GAN"), P("optim"), P("steps")
    G = P("models.GAN.generator")
    perc = GANu.PerceptualLoss(resize_to=32, crop=28).to(dev)
    lr = filler.tensor("in:ema_gan_lr", (4, 3, 16, 16), 0.5, 0.5).to(dev)
    hr = filler.tensor("in:ema_gan_hr", (4, 3, 64, 64)).to(dev)

    def make():
        g, d = G.Generator(4, 2), Dm.Discriminator((64, 64))
        g.load_state_dict(filler.fill_state_dict(gan.template(gan.generator_shapes(4, 2))))
        d.load_state_dict(filler.fill_state_dict(gan.template(gan.discriminator_shapes((64, 64)))))
        g.to(dev).train(), d.to(dev).train()
        return g, d, O.FusedAdam(g.parameters(), lr=1e-3), O.FusedAdam(d.parameters(), lr=1e-3)

    g, d, og, od = make()
    ema = O.WeightEMA(g, decay=0.9)
    start, snaps = _clone(g), []
    for _ in range(2):
        out = S.gan_step(g, d, perc, og, od, lr, hr, ema=ema)
        snaps.append(_clone(g))
    _check_against_ref(ema, g, start, snaps, label="gan_step")
    assert not same(ema.state_dict()["shadow"]["conv3.weight"], g.conv3.weight)
    # the same two steps without an EMA: both networks and the step's outputs are bit for bit what they were
    g2, d2, og2, od2 = make()
    for _ in range(2):
        out2 = S.gan_step(g2, d2, perc, og2, od2, lr, hr)
    torch.cuda.synchronize()
    for a, b in zip(out, out2):
        assert same(a, b)
    for ma, mb in ((g, g2), (d, d2)):
        for (k, a), (_, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert same(a, b), k


def test_state_round_trip(dev, trained):
    O = P("optim")
    g, ema = trained["gen"], trained["ema"]
    twin = O.WeightEMA(g, decay=0.5, warmup=True)
    twin.load_state_dict(ema.state_dict())
    assert (twin.decay, twin.warmup, twin.use_buffers) == (ema.decay, ema.warmup, ema.use_buffers)
    assert twin.n_averaged.item() == ema.n_averaged.item() == 6
    assert all(same(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(twin._shadow, ema._shadow))
    keep = ema.state_dict()
    try:
        with torch.no_grad():
            for p in g.parameters():
                p.mul_(1.01)
        ema.update()
        twin.update()
        torch.cuda.synchronize()
        assert twin.n_averaged.item() == ema.n_averaged.item() == 7
        assert all(same(a, b) for a, b in zip(twin._shadow, ema._shadow))
        assert not same(ema._shadow[0], keep["shadow"]["conv1.weight"])
    finally:
        with torch.no_grad():
            for p, q in zip(g.parameters(), trained["snaps"][-1].values()):
                p.copy_(q)
        ema.load_state_dict(keep)
