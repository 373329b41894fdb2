"""CPU: tests/adam_sweep_ref.py itself.  The one-step reference against clip_ref.ClippedAdam and torch.optim.Adam in float64;
an fp32 op-by-op emulation of adam_update / adam_coef inside every band for every case of the tables; every listed wrong
variant outside them; every case past the threshold it is named for; no subnormal intermediate."""
import numpy as np
import pytest
import torch

import adam_sweep_ref as R
import clip_ref


def _np(xs):
    return [x.numpy() for x in xs]


@pytest.fixture(scope="module")
def data():
    """Inputs of every case, drawn once and left unchanged.  The case past the grid cap is sampled at 200 000 elements with
    its own mode, step and set (its 134 M elements are generated, and checked, on the device only)."""
    d = {c.name: R.case_data(c) for c in R.PW_CASES + R.MT_CASES}
    d[R.BIG_CASE.name] = [R.draw(200_000, R.BIG_CASE.seed, R.BIG_CASE.mode["S"])]
    return d


ALL_CASES = R.PW_CASES + R.MT_CASES + [R.BIG_CASE]


# ----------------------------------------------------------------------------- the reference
def test_rotation_covers_every_mode_step_pair():
    pairs = {(c.mode["name"], c.t) for c in R.PW_CASES}
    assert len(pairs) == 25
    assert {c.lr for c in ALL_CASES} == {R.F32(1e-2), R.F32(1e-4)} and {c.b2 for c in ALL_CASES} == {R.F32(0.999), R.F32(0.99)}
    assert {c.mode["name"] for c in R.MT_CASES} == {"host_gs", "hyper", "scaler", "found0"}
    assert R.BIG_CASE.t == 1000 and R.BIG_CASE.shadow and R.BIG_CASE.mode["name"] == "hyper"
    # the multipliers: exact powers of two, and the one fp32 product of the hyper mode
    gs = {m["name"]: R.multiplier(m) for m in R.MODES}
    assert gs["host"] == gs["found0"] == 1.0 and gs["host_gs"] == 2.0 ** -10 and gs["scaler"] == 2.0 ** -16
    assert gs["hyper"] == float(np.float32(2.0 ** -10) * np.float32(0.37))
    for m in R.MODES:                               # the true gradient is raw * (multiplier without the coefficient)
        assert m["S"] * (R.multiplier(m) / (R.F32(R.COEF) if m.get("hyper") else 1.0)) == 1.0


@pytest.mark.parametrize("t", [1, 2, 7, 1000])
def test_adam_step_against_clipped_adam_and_torch(t):
    """One step from a state in the middle of a run.  clip_ref.ClippedAdam is given the state and t - 1 (its betas rounded to
    fp32); torch.optim.Adam in float64 gets the same state through its state dict.  1e-12 relative, elementwise."""
    lr, b1, b2, eps = (R.F32(x) for x in R.SETS[t % 2])
    p, g, m, v, _ = R.draw(4099, 5 + t, 1.0)
    keep = v > 0                                    # (torch's Adam and the reference agree at v = 0 too; relative needs p' != 0)
    p1, m1, v1 = R.adam_step(p, g, m, v, t, lr, b1, b2, eps, 0.25)
    ca = clip_ref.ClippedAdam([p.numpy()], lr=lr, betas=(b1, b2), eps=eps, grad_scale=0.25)
    ca.m, ca.v, ca.t = [m.double().numpy().copy()], [v.double().numpy().copy()], t - 1
    ca.step([g.numpy()])
    for got, want in ((ca.p[0], p1), (ca.m[0], m1), (ca.v[0], v1)):
        want = want.numpy()
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[w] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    w.grad = g.double() * 0.25
    opt.step()
    for got, want in ((w.detach(), p1), (opt.state[w]["exp_avg"], m1), (opt.state[w]["exp_avg_sq"], v1)):
        assert bool(((got - want).abs() <= 1e-12 * want.abs()).all())
    assert bool(keep.any())


def test_every_regime_occurs_and_zero_regime_is_exact(data):
    for c in R.PW_CASES[-2:] + R.MT_CASES[1:]:
        seen = torch.cat([d[4] for d in data[c.name]]).bincount(minlength=7)
        assert bool((seen > 0).all()), c
    p, g, m, v, r = data[R.PW_CASES[-1].name][0]
    z = r == R.ALL_ZERO
    assert bool((g[z] == 0).all() and (m[z] == 0).all() and (v[z] == 0).all())
    assert bool((g[r == R.G_ZERO] == 0).all() and (v[r == R.G_ZERO] > 0).all())
    assert bool((p[r == R.P_ZERO] == 0).all())
    tiny = g[r == R.TINY].abs() / R.PW_CASES[-1].mode["S"]
    assert 1e-9 * 0.999 <= tiny.min() and tiny.max() <= 1e-6 * 1.001
    assert g[r == R.LARGE].abs().min() >= 1e12 * R.PW_CASES[-1].mode["S"]


# ----------------------------------------------------------------------------- the emulation is inside every band
def _case_ratios(c, dat, variant=None):
    """Per tensor: (ratio_p, ratio_m, ratio_v, zero_ok, shadow bits of the emulation, its p, regime)."""
    out = []
    for p, g, m, v, r in dat:
        ep, em, ev, sh = R.emulate_launch(*_np((p, g, m, v)), c.hyp(), variant)
        got = tuple(torch.from_numpy(x) for x in (ep, em, ev))
        rp, rm, rv, zok = R.compare(got, (p, g, m, v), r, c.hyp())
        out.append((rp, rm, rv, zok, torch.from_numpy(sh), got[0], r))
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_fp32_emulation_is_inside_every_band(case, data):
    worst = [0.0, 0.0, 0.0]
    for rp, rm, rv, zok, sh, p1, _ in _case_ratios(case, data[case.name]):
        assert zok
        assert bool((sh == R.bf16_bits(p1)).all())                  # the emulation's rounding IS torch's bf16 cast
        for i, r in enumerate((rp, rm, rv)):
            worst[i] = max(worst[i], float(r.max()))
    print(f"{case!r}: worst |delta|/band  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


# ----------------------------------------------------------------------------- every wrong variant is outside
def _designated(variant):
    """(cases, regimes whose elements must leave the band) for a variant."""
    pw = [c for c in R.PW_CASES if c.sizes[0] >= 1023] + R.MT_CASES[1:]
    if variant in ("eps_in_root", "eps_before_bc"):
        return [c for c in pw if c.t <= 10], (R.TINY,)
    if variant in ("t+1", "t-1"):                                    # (at b2 = 0.99, t = 1000 the two differ by 4e-7 of b2^t: inside)
        return [c for c in pw if c.t <= 7 or (c.t == 1000 and c.b2 > 0.995)], (R.NORMAL, R.P_ZERO, R.P_SMALL, R.TINY, R.LARGE)
    if variant == "v_g_gk":
        return [c for c in pw if c.gs != 1.0], (R.NORMAL, R.P_ZERO, R.P_SMALL, R.TINY, R.LARGE)
    return pw, (R.NORMAL, R.P_ZERO, R.P_SMALL, R.LARGE)


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if not v.startswith(("tail", "shadow"))])
def test_arithmetic_variants_leave_the_bands(variant, data):
    """More than 2x outside a band for at least 80 % of the elements of the relevant regimes, in every designated case."""
    cases, regimes = _designated(variant)
    assert cases
    for c in cases:
        rs = _case_ratios(c, data[c.name], variant)
        worst = torch.cat([torch.maximum(torch.maximum(rp, rm), rv) for rp, rm, rv, *_ in rs])
        r = torch.cat([x[6] for x in rs])
        sel = torch.zeros_like(r, dtype=torch.bool)
        for k in regimes:
            sel |= r == k
        assert int(sel.sum()) >= 100, c
        frac = float((worst[sel] > 2.0).float().mean())
        print(f"{variant} {c!r}: {100 * frac:.1f} % of {int(sel.sum())} elements more than 2x outside")
        assert frac >= 0.8, (variant, c, frac)


def test_tail_variants_leave_the_bands(data):
    """A tail element left alone or updated twice: every tail element outside the all-zero regime is more than 2x outside."""
    cases = [c for c in R.PW_CASES if c.sizes[0] % 4 and c.sizes[0] > 4]
    assert len(cases) >= 12
    for variant in ("tail_skipped", "tail_twice"):
        hit = 0
        for c in cases:
            n = c.sizes[0]
            (rp, rm, rv, _, _, _, r), = _case_ratios(c, data[c.name], variant)
            worst = torch.maximum(torch.maximum(rp, rm), rv)
            assert float(worst[:n - n % 4].max()) <= 1.0                  # the body is the right one
            live = r[n - n % 4:] != R.ALL_ZERO
            assert bool((worst[n - n % 4:][live] > 2.0).all()), (variant, c)
            hit += int(live.sum())
        assert hit >= 12


def test_shadow_variants_differ_from_the_rounded_image(data):
    cases = [c for c in R.PW_CASES if c.shadow and c.sizes[0] >= 1023]
    for variant in ("shadow_truncated", "shadow_old_p"):
        for c in cases:
            (_, _, _, _, sh, p1, r), = _case_ratios(c, data[c.name], variant)
            diff = sh != R.bf16_bits(p1)
            assert float(diff.float().mean()) > 0.2, (variant, c)
            n = c.sizes[0]
            if n % 4 and variant == "shadow_truncated":                   # whole-tensor comparison sees a wrong tail image too
                assert diff.numel() == n


# ----------------------------------------------------------------------------- every case is past its threshold
def test_pw_cases_are_past_their_thresholds():
    want = {        # n: (blocks, passes, [(u0, u1) vectors per block of the last pass], tail)
        1: (1, 0, [], 1), 2: (1, 0, [], 2), 3: (1, 0, [], 3),                      # the tail alone
        4: (1, 1, [(1, 0)], 0), 5: (1, 1, [(1, 0)], 1), 7: (1, 1, [(1, 0)], 3),
        1023: (1, 1, [(255, 0)], 3),
        1024: (1, 1, [(256, 0)], 0),                                               # n/4 = 256: the u = 1 half is empty
        1028: (1, 1, [(256, 1)], 0),                                               # n/4 = 257: one u = 1 vector
        2047: (1, 1, [(256, 255)], 3),
        2048: (1, 1, [(256, 256)], 0),                                             # one full block
        2052: (2, 1, [(256, 256), (1, 0)], 0),                                     # the second block
        4099: (2, 1, [(256, 256), (256, 256)], 3),
        13317: (7, 1, [(256, 256)] * 6 + [(256, 1)], 1),
        (1 << 20) + 3: (512, 1, [(256, 256)] * 512, 3),
    }
    assert set(want) == set(R.PW_SIZES)
    for n, (blocks, passes, halves, tail) in want.items():
        geo = R.pw_geometry(n)
        assert (geo["blocks"], geo["passes"], geo["halves"], geo["tail"]) == (blocks, passes, halves, tail), n
    assert {c.sizes[0] for c in R.PW_CASES if c.shadow} == {c.sizes[0] for c in R.PW_CASES if not c.shadow} == set(R.PW_SIZES)
    # past the grid cap: the second pass has block 0 with both halves, block 1 with a full u = 0 half and one u = 1 vector
    geo = R.pw_geometry(R.BIG_N)
    assert R.BIG_N == 134_220_807 and R.BIG_N > 65536 * 2048
    assert (geo["blocks"], geo["passes"], geo["halves"], geo["tail"]) == (65536, 2, [(256, 256), (256, 1)], 3)


def test_mt_tables_are_past_their_thresholds():
    assert [len(c.sizes) for c in R.MT_CASES] == [1, 64, 65, 129]
    for c in R.MT_CASES:
        groups = R.mt_groups(c.sizes)
        assert len(groups) == -(-len(c.sizes) // 64)
        for slot in (0, 63, 64):
            if slot < len(c.sizes):
                assert c.sizes[slot] == 40961
        first, grid = groups[0]
        assert first[0] == 0 and (len(first) == 1 or first[1] == 11)              # 40961 elements = 11 blocks of 4096
        assert grid == sum(-(-n // 4096) for n in c.sizes[:64])
        if len(c.sizes) > 64:                                                     # multi-block tensors on both sides of the boundary
            assert first[63] == grid - 11 and groups[1][0][0] == 0
            assert groups[1][1] >= 11 and (len(groups[1][0]) == 1 or groups[1][0][1] == 11)
        # every p, g, m, v takes every offset, independently
        for k in range(4):
            assert {o[k] for o in c.offs} == ({0, 4, 8, 12} if len(c.sizes) > 1 else {c.offs[0][k]})
        if len(c.sizes) >= 64:
            assert len(set(c.offs[:64])) == 64
    big = R.MT_CASES[-1]
    assert set(big.sizes) == set(R.MT_SIZES) and len(R.mt_groups(big.sizes)) == 3
    assert len(R.mt_groups(big.sizes)[2][0]) == 1                                  # the third launch carries one tensor
    # sizes on both sides of the 256-thread stride and of the 4096 chunk
    assert {255, 256, 257, 4095, 4096, 4097, 8192, 8193} <= set(R.MT_SIZES)


# ----------------------------------------------------------------------------- no subnormal intermediate
@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_no_intermediate_is_subnormal(case, data):
    """Every intermediate of the reference is 0 or at least 1e-30 in magnitude (fp32's smallest normal is 1.2e-38), so the
    relative bands apply.  m' is exempt below that by cancellation only: an fp32 sum that lands there is exact."""
    h = case.hyp()
    for p, g, m, v, _ in data[case.name]:
        p, g, m, v = (x.double() for x in (p, g, m, v))
        gk = g * h["gs"]
        v1 = h["b2"] * v + (1 - h["b2"]) * gk * gk
        m1 = h["b1"] * m + (1 - h["b1"]) * gk
        D = v1.sqrt() / (1 - h["b2"] ** h["t"]) ** 0.5 + h["eps"]
        q = m1 / D
        for name, x in (("g", g), ("gk", gk), ("b1 m", h["b1"] * m), ("w1 gk", (1 - h["b1"]) * gk), ("b2 v", h["b2"] * v),
                        ("w2 gk", (1 - h["b2"]) * gk), ("w2 gk gk", (1 - h["b2"]) * gk * gk), ("v'", v1), ("sqrt", v1.sqrt()),
                        ("D", D), ("m/D", q), ("U", h["lr"] / (1 - h["b1"] ** h["t"]) * q)):
            a = x.abs()
            ok = (a == 0) | (a >= 1e-30)
            if name in ("m/D", "U"):
                ok |= (m1.abs() < 1e-30)
            assert bool(ok.all()) and bool((a < 3e38).all()), (case, name)
