"""CPU: the reference of the pass-by-pass L-BFGS sweep (tests/lbfgs_ref.py) against itself and against torch.

The device test (test_gpu_lbfgs_passes.py) bounds every element of the pending s of one pass by
    |s_dev - s64| <= 2^-24 |s64| + KAPPA 2^-53 A,    s64 = t d from two_loop_direction, A = t sum_l |coef_l| |v_l|.
Here, with no device: kappa_0 (the Gram form against the vector form, both float64 numpy) is measured over the whole case
table and held against the constant KAPPA0 that the bound is built on; the bound is shown not to be vacuous (median relative width
<= 2^-23 in every pass) and to discriminate (four deliberate errors of the Gram form exceed it >= 100 x); and
two_loop_direction is anchored to torch.optim.LBFGS's own d."""
import numpy as np
import pytest
import torch

import lbfgs_ref as R


@pytest.fixture(scope="module")
def sweep():
    """Every case driven by the teacher-forced driver alone, its own fp32-rounded outputs as the next stored state; per
    case the list of per-pass expectations."""
    out = {}
    for name, case in R.CASES.items():
        rec = []
        R.run_case(case, R.HostBackend(), lambda i, exp, before, after, g32: rec.append(exp))
        out[name] = rec
    return out


def test_kappa0_gram_form_against_vector_form(sweep):
    """kappa_0 = max |s_gram - s_vec| / (2^-53 A) over all cases, passes and elements (elements with A = 0 must agree exactly:
    both forms sum zeros there)."""
    worst = {}
    for name, rec in sweep.items():
        k = 0.0
        for exp in rec:
            if exp["mode"] == 0 or np.isnan(exp["s64"]).any():
                continue
            diff, a = np.abs(exp["s_gram"] - exp["s64"]), R.U53 * exp["A"]
            assert (diff[a == 0] == 0).all()
            k = max(k, float((diff[a > 0] / a[a > 0]).max()))
        worst[name] = k
        print(f"{name:18s} kappa_0 = {k:.3f}")
    k0 = max(worst.values())
    print(f"kappa_0 = {k0:.3f} (constant in lbfgs_ref.py: {R.KAPPA0}, device bound uses KAPPA = {R.KAPPA})")
    assert R.KAPPA == 4 * R.KAPPA0
    assert R.KAPPA0 / 2 <= k0 <= 2 * R.KAPPA0, "KAPPA0 is the figure measured here (to the BLAS's summation order)"


def test_case_table_reaches_what_it_claims(sweep):
    live = [e["hdr"][4] for e in sweep["trips_m70"]]
    assert live == [min(i, 70) for i in range(76)], "every pair of the m = 70 case commits; five wraps"
    assert [e["hdr"][4] for e in sweep["ring_m1"]] == [0, 1, 1, 1, 1, 1]
    assert [e["hdr"][4] for e in sweep["ring_m2"]] == [0, 1, 2, 2, 2, 2, 2, 2, 2]
    assert [e["hdr"][4] for e in sweep["max_history"]] == list(range(6))
    last = {n: (r[-1]["mode"], r[-1]["stop"]) for n, r in sweep.items()}
    for name in ("exit_first_grad", "exit_max_eval", "exit_grad_later", "exit_step_size", "exit_loss_change"):
        assert last[name] == (0, 1), name
        assert all(e["stop"] == 0 and e["mode"] == 2 for e in sweep[name][:-1]), name
    assert sweep["exit_first_grad"][0]["hdr"] == [0, 1, 0, 1, 0]
    assert sweep["exit_max_eval"][-1]["hdr"] == [2, 3, 2, 3, 1]
    assert last["exit_max_iter"] == (2, 1) and sweep["exit_max_iter"][-1]["hdr"] == [3, 3, 3, 3, 2]
    g = sweep["exit_gtd"]
    assert [(e["mode"], e["stop"], e["committed"], e["hdr"][4]) for e in g] == [(1, 1, False, 0), (1, 1, True, 1)]
    d = sweep["dropped_pair"]
    assert [e["committed"] for e in d] == [False, True, True, False, True] and d[3]["ys"] == 0.0
    assert [e["hdr"][4] for e in d] == [0, 1, 2, 2, 3]
    t = sweep["two_steps"]
    assert [e["stop"] for e in t] == [0, 0, 1, 0, 0, 1] and t[-1]["hdr"] == [6, 6, 3, 3, 3]
    n = sweep["nan"]
    assert [e["hdr"][4] for e in n] == [0, 0, 1, 2, 2, 2]
    assert [int(np.isnan(e["s64"]).sum()) for e in n] == [1, 0, 0, 0, 12, 0]
    assert all(np.array_equal(np.isnan(e["s64"]), np.isnan(e["s_gram"])) for e in n)


def test_bound_is_not_vacuous(sweep):
    """Median over the elements (those with s64 != 0) of bound / |s64| <= 2^-23 in every case and pass: at least half of the
    elements are held to within two fp32 roundings."""
    worst = 0.0
    for name, rec in sweep.items():
        meds = []
        for exp in rec:
            if exp["mode"] == 0 or np.isnan(exp["s64"]).any():
                continue
            nz = exp["s64"] != 0
            meds.append(float(np.median(R.bound(exp)[nz] / np.abs(exp["s64"][nz]))))
        if meds:
            print(f"{name:18s} median bound / |s64|: worst pass {max(meds) * 2 ** 24:.4f} x 2^-24")
            worst = max(worst, max(meds))
            assert max(meds) <= 2.0 ** -23, name
    assert worst > 0


@pytest.mark.parametrize("corrupt,at", [("stale", 45), ("lane64", 45), ("evicted", 72), ("h_diag", 45)])
def test_bound_discriminates(sweep, corrupt, at):
    """One error in one pass of the Gram form at k >= 40 live pairs (m = 70 case): the pass's s leaves the bound by >= 100 x on
    some element.  The state before the pass is the clean run's."""
    clean = sweep["trips_m70"]
    rec = []
    R.run_case(R.CASES["trips_m70"], R.HostBackend(), lambda i, exp, before, after, g32: rec.append(exp),
               driver=lambda n, **kw: R.CorruptedDriver(n, corrupt, at, **kw))
    assert clean[at]["hdr"][4] >= 40 and clean[at]["committed"]
    assert np.array_equal(rec[at - 1]["s_gram"], clean[at - 1]["s_gram"])
    ratio = float((np.abs(rec[at]["s_gram"] - clean[at]["s64"]) / R.bound(clean[at])).max())
    print(f"{corrupt}: pass {at}, k = {clean[at]['hdr'][4]}: worst |s - s64| / bound = {ratio:.3e}")
    assert ratio >= 100


@pytest.mark.parametrize("iters", [3, 40, 110])
def test_two_loop_direction_reproduces_torch(iters):
    """torch.optim.LBFGS in float64 on the quadratic of test_host_lbfgs.py (n = 5000, history 100): after `iters` iterations
    its state (old_dirs, old_stps, H_diag and the gradient d was built from, kept as prev_flat_grad) gives torch's d to
    1e-12 relative."""
    rng = np.random.default_rng(0)
    ev, b = torch.tensor(np.logspace(0, 3, 5000)), torch.tensor(rng.standard_normal(5000))
    x = torch.tensor(rng.standard_normal(5000)).requires_grad_(True)
    opt = torch.optim.LBFGS([x], lr=1, max_iter=iters, max_eval=10 ** 6, tolerance_grad=-1, tolerance_change=-1,
                            history_size=100)

    def closure():
        opt.zero_grad()
        loss = 0.5 * (ev * x * x).sum() - (b * x).sum()
        loss.backward()
        return loss

    opt.step(closure)
    st = opt.state[opt._params[0]]
    assert st["n_iter"] == iters and len(st["old_dirs"]) == min(iters - 1, 100)      # no pair was skipped
    S = np.stack([v.numpy() for v in st["old_stps"]])
    Y = np.stack([v.numpy() for v in st["old_dirs"]])
    d = R.two_loop_direction(S, Y, st["prev_flat_grad"].numpy(), float(st["H_diag"]))
    want = st["d"].numpy()
    err = float(np.linalg.norm(d - want) / np.linalg.norm(want))
    print(f"{iters} iterations, {len(S)} pairs: relative difference {err:.3e}")
    assert err <= 1e-12
