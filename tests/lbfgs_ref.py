"""float64 numpy model of the vector-free L-BFGS that csrc/lbfgs.hip implements (Chen, Wang & Zhou, NIPS 2014).

Same state machine as the kernels: m + 1 ring slots, the pending pair (s = t d, y = g - g_prev) kept in the free slot until
the next iteration commits it (ys > 1e-10) or drops it, a Gram matrix over the basis {S slots, Y slots, g} updated only
with the dots of the pending pair and the new gradient, the two-loop recursion on coefficients, and every break of
torch/optim/lbfgs.py decided from scalars.  Only the four passes' arithmetic differs: here dots and combinations are
plain float64 numpy.

The second half of the file is the pass-by-pass reference: two_loop_direction (the recursion on the vectors themselves, the
independent yardstick), a teacher-forced driver, the per-element bound, and the case table both pass tests run."""
import numpy as np


class GramLBFGS:
    def __init__(self, n, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                 history_size=100):
        self.n, self.m = n, history_size
        self.lr, self.max_iter = lr, max_iter
        self.max_eval = max_iter * 5 // 4 if max_eval is None else max_eval
        self.tol_grad, self.tol_change = tolerance_grad, tolerance_change
        m = history_size
        self.S = np.zeros((m + 1, n))
        self.Y = np.zeros((m + 1, n))
        self.gbuf = np.zeros((2, n))
        self.nb = 2 * (m + 1) + 1
        self.gram = np.zeros((self.nb, self.nb))
        self.ro = np.zeros(m + 1)
        self.slot_of = []
        self.free = 0
        self.gprev = 0
        self.n_iter = self.func_evals = 0
        self.h_diag = 1.0
        self.t = 0.0
        self.prev_loss = 0.0
        self.dt_max = 0.0

    def _vec(self, c, gcur):
        m = self.m
        if c < m + 1:
            return self.S[c]
        if c < 2 * (m + 1):
            return self.Y[c - m - 1]
        return self.gbuf[gcur]

    def _pending_y(self, g, g_prev):
        return g - g_prev

    def _commit(self, p, pend, dots):
        """ys > 1e-10: the pending pair's Gram entries, ro and h_diag, then the ring (a full ring evicts its oldest slot)."""
        m = self.m
        for j in self.slot_of:
            d = dots[j]
            for (a, b), v in zip(((p, j), (p, m + 1 + j), (m + 1 + p, j), (m + 1 + p, m + 1 + j)), d[:4]):
                self.gram[a, b] = self.gram[b, a] = v
        self.gram[p, p] = pend[0]
        self.gram[p, m + 1 + p] = self.gram[m + 1 + p, p] = pend[1]
        self.gram[m + 1 + p, m + 1 + p] = pend[2]
        self.ro[p] = 1.0 / pend[1]
        self.h_diag = pend[1] / pend[2]
        if len(self.slot_of) == m:
            ev = self.slot_of.pop(0)
            self.slot_of.append(p)
            self.free = ev
        else:
            self.slot_of.append(p)
            self.free = len(self.slot_of)

    def _rdot(self, q, lst, row):
        """One dot of the recursion: the coefficient vector against a Gram row, over the live indices."""
        return q[lst] @ self.gram[row, lst]

    def _recursion(self, lst, k):
        """The two-loop recursion on coefficients over the Gram indices lst = [S slots, Y slots, G]; returns q [nb]."""
        G = 2 * (self.m + 1)
        q = np.zeros(self.nb)
        q[G] = -1.0
        al = [0.0] * k
        for i in range(k - 1, -1, -1):
            al[i] = self._rdot(q, lst, lst[i]) * self.ro[lst[i]]
            q[lst[k + i]] -= al[i]
        q[lst] *= self.h_diag
        for i in range(k):
            be = self._rdot(q, lst, lst[k + i]) * self.ro[lst[i]]
            q[lst[i]] += al[i] - be
        return q

    def _pass(self, loss, g, first):
        """gather + dots + scalar + combine for one closure value; returns (stop, update) where update is the
        parameter increment (None when the parameters do not move).  self.last records what the pass decided: mode (0 nothing
        written, 1 the pending s only, 2 and the parameters), committed, and for mode != 0 the Gram indices lst, their
        coefficients coef, the gradient buffer gcur and gtd."""
        m, G = self.m, 2 * (self.m + 1)
        # gather
        gcur = 1 - self.gprev
        p = self.free
        self.gbuf[gcur] = g
        self.Y[p] = self._pending_y(g, self.gbuf[self.gprev])
        gmax, gsum = np.abs(g).max(), np.abs(g).sum()
        # dots
        sp, yp = self.S[p], self.Y[p]
        pend = [sp @ sp, sp @ yp, yp @ yp, g @ sp, g @ yp, g @ g]
        dots = {j: (sp @ self.S[j], sp @ self.Y[j], yp @ self.S[j], yp @ self.Y[j], g @ self.S[j], g @ self.Y[j])
                for j in self.slot_of}
        # scalar
        opt_cond = gmax <= self.tol_grad
        if first:
            self.n_iter_step, self.cur_evals = 0, 1
            self.func_evals += 1
            stop = opt_cond
        else:
            self.cur_evals += 1
            self.func_evals += 1
            stop = (self.cur_evals >= self.max_eval or opt_cond or self.dt_max <= self.tol_change
                    or abs(loss - self.prev_loss) < self.tol_change)
        if not stop and self.n_iter_step >= self.max_iter:
            stop = True
        self.last = dict(mode=0, committed=False, gmax=gmax, ys=pend[1])
        if stop:
            return True, None
        self.n_iter_step += 1
        self.n_iter += 1
        committed = False
        if self.n_iter == 1:
            self.slot_of, self.free, self.h_diag = [], 0, 1.0
        elif pend[1] > 1e-10:
            committed = True
            self._commit(p, pend, dots)
        k = len(self.slot_of)
        for j in self.slot_of:
            gs, gy = (pend[3], pend[4]) if committed and j == p else dots[j][4:]
            self.gram[G, j] = self.gram[j, G] = gs
            self.gram[G, m + 1 + j] = self.gram[m + 1 + j, G] = gy
        self.gram[G, G] = pend[5]
        lst = list(self.slot_of) + [m + 1 + j for j in self.slot_of] + [G]
        q = self._recursion(lst, k)
        gtd = q[lst] @ self.gram[G, lst]
        d = sum(q[c] * self._vec(c, gcur) for c in lst)
        self.gprev = gcur
        self.prev_loss = loss
        if self.n_iter == 1:
            x = 1.0 / gsum
            self.t = (x if x < 1.0 else 1.0) * self.lr
        else:
            self.t = self.lr
        # combine
        s = self.t * d
        self.S[self.free] = s
        self.last.update(mode=1, committed=committed, lst=lst, coef=q[lst], gcur=gcur, gtd=gtd)
        if gtd > -self.tol_change:
            return True, None
        self.last["mode"] = 2
        self.dt_max = np.abs(s).max()
        return self.n_iter_step == self.max_iter, s

    def step(self, x, closure):
        """closure(x) -> (loss, flat gradient); x (float64, updated in place).  Returns (first loss, closure calls)."""
        loss, g = closure(x)
        first_loss, calls = loss, 1
        stop, upd = self._pass(float(loss), g, True)
        if upd is not None:
            x += upd
        while not stop:
            loss, g = closure(x)
            calls += 1
            stop, upd = self._pass(float(loss), g, False)
            if upd is not None:
                x += upd
        return first_loss, calls


# ---------------------------------------------------------------------------------------------------------------------
# Pass-by-pass checking (tests/test_host_lbfgs_passes.py on the CPU, tests/test_gpu_lbfgs_passes.py on the device).
#
# The yardstick of one pass is two_loop_direction on the stored vectors themselves; the driver below holds only the
# bookkeeping and is handed the stored fp32 vectors before every pass, so no rounding compounds and every bound is a bound on
# one pass:   |s - s64| <= 2^-24 |s64| + KAPPA 2^-53 A,   A = t sum_l |coef_l| |v_l|   (Gram-form coefficients),
# one fp32 rounding of the stored s plus KAPPA fp64 roundings of the magnitude that the combination sums.

U24, U53 = 2.0 ** -24, 2.0 ** -53

# kappa_0: the largest |s_gram - s_vec| / (2^-53 A) over every case, pass and element of CASES, the Gram form (GramLBFGS,
# teacher-forced) against two_loop_direction, both in numpy float64.  Measured by
#     python -m pytest tests/test_host_lbfgs_passes.py -s -k kappa0
# which printed kappa_0 = 10.886 (the m = 70 case; 10.426 on the 133121-element one, below 5 elsewhere).  The figure is a
# maximum of rounding noise, so another BLAS may sum in another order and print a slightly different one; that test holds
# the constant to within a factor 2 of what it measures.  The device bound uses 4 kappa_0: the factor 4 is for the kernels'
# summation order (per-thread fma chains, butterfly, blocks in order), which is not numpy's.
KAPPA0 = 10.886
KAPPA = 4.0 * KAPPA0


def two_loop_direction(S, Y, g, h_diag):
    """The two-loop recursion of torch/optim/lbfgs.py:423-442 on the vectors themselves, float64: S, Y [k, n] the pairs in age
    order (oldest first), g [n]; returns d = -H g.  No Gram matrix, nothing from the package."""
    S, Y = np.asarray(S, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    k = len(S)
    q = -np.asarray(g, dtype=np.float64)
    ro = [1.0 / (Y[i] @ S[i]) for i in range(k)]
    al = [0.0] * k
    for i in range(k - 1, -1, -1):
        al[i] = (S[i] @ q) * ro[i]
        q = q - al[i] * Y[i]
    r = q * h_diag
    for i in range(k):
        be = (Y[i] @ r) * ro[i]
        r = r + (al[i] - be) * S[i]
    return r


def clear_of(value, threshold):
    """A decision `value <=> threshold` is not within rounding: the two differ by a factor >= 2 (or in sign).  A NaN value
    decides every comparison as false on both sides."""
    return bool(np.isnan(value) or abs(value - threshold) >= 0.5 * max(abs(value), abs(threshold)))


class PassDriver(GramLBFGS):
    """GramLBFGS's bookkeeping (slot_of, free slot, gprev, h_diag, t, prev_loss, the four counters, dt_max, live pairs),
    teacher-forced: expect() is handed the stored fp32 ring and gradient buffers (as float64) before each pass."""

    def __init__(self, n, **kw):
        super().__init__(n, **kw)
        self.n_iter_step = self.cur_evals = 0

    def _pending_y(self, g, g_prev):         # the gather pass: one fp32 subtraction
        return (g.astype(np.float32) - g_prev.astype(np.float32)).astype(np.float64)

    def expect(self, S, Y, gbuf, g, loss, first):
        """One pass over the stored state S, Y [m + 1, n], gbuf [2, n] with gradient g [n] (fp32 values) and loss.  Returns a
        dict: p (the slot the pending y goes to), gcur, y, committed, mode, stop, hdr (the five header ints), free (the slot
        of the pending s afterwards), margins [(name, value, threshold)] of every decision taken, and for mode != 0 s64
        (t d, d from two_loop_direction), s_gram (the Gram form's), A."""
        self.S[:], self.Y[:], self.gbuf[:] = S, Y, gbuf
        p, gcur, prev_loss = self.free, 1 - self.gprev, self.prev_loss
        self.dt_max = float(np.abs(self.S[p]).max())       # max|s| of the stored pending s, what the combine pass keeps
        n_iter_before = self.n_iter
        stop, _ = self._pass(float(loss), g, bool(first))
        last = self.last
        margins = [("max|g| <= tolerance_grad", last["gmax"], self.tol_grad)]
        if not first:
            margins += [("max|t d| <= tolerance_change", self.dt_max, self.tol_change),
                        ("|loss - prev_loss| < tolerance_change", abs(float(loss) - prev_loss), self.tol_change)]
        out = dict(p=p, gcur=gcur, y=self.Y[p].copy(), committed=last["committed"], mode=last["mode"], stop=int(stop),
                   free=self.free, hdr=[self.n_iter, self.func_evals, self.n_iter_step, self.cur_evals, len(self.slot_of)],
                   margins=margins, ys=None)
        if last["mode"] == 0:
            return out
        if n_iter_before >= 1:
            out["ys"] = last["ys"]
        margins.append(("gtd > -tolerance_change", last["gtd"], -self.tol_change))
        lst, coef = last["lst"], last["coef"]
        d = two_loop_direction(self.S[self.slot_of], self.Y[self.slot_of], g, self.h_diag)
        out["s64"] = self.t * d
        out["s_gram"] = self.S[self.free].copy()
        out["A"] = self.t * sum(abs(c) * np.abs(self._vec(ci, gcur)) for c, ci in zip(coef, lst))
        return out


def decisions_clear(exp):
    """No decision of the pass sits within rounding of its threshold: ys is exactly 0 or at least 1e-6 away from 1e-10, every
    other quantity a factor >= 2 away from its tolerance."""
    ys = exp["ys"]
    bad = [m for m in exp["margins"] if not clear_of(m[1], m[2])]
    if ys is not None and not (np.isnan(ys) or ys == 0.0 or abs(ys - 1e-10) >= 1e-6):
        bad.append(("ys > 1e-10", ys, 1e-10))
    return bad


def bound(exp):
    """The per-element bar on the pending s of one pass."""
    return U24 * np.abs(exp["s64"]) + KAPPA * U53 * exp["A"]


class CorruptedDriver(PassDriver):
    """PassDriver with one deliberate error of the Gram form, for the test that the bound discriminates:
    'stale'   one s_j . y_p entry (p the committed slot, j an older live one) is not written on a commit -- the recursion
              reads s_older . y_newer only, so the s_p . y_j entries of the same commit could be stale unnoticed,
    'lane64'  the recursion's first dot drops the terms with list index >= 64,
    'evicted' after a wrap the newest live entry names the evicted slot instead of the committed one,
    'h_diag'  a commit does not update h_diag."""
    def __init__(self, n, corrupt, at, **kw):
        """The error is made in pass number `at` (counted from 0) alone."""
        super().__init__(n, **kw)
        self.corrupt, self.at = corrupt, at

    def _now(self, kind):
        return self.corrupt == kind and self.func_evals == self.at + 1

    def _commit(self, p, pend, dots):
        m, h, full = self.m, self.h_diag, len(self.slot_of) == self.m
        j0 = self.slot_of[len(self.slot_of) // 2] if self.slot_of else p
        old = self.gram[j0, m + 1 + p]
        super()._commit(p, pend, dots)
        if self._now("stale"):
            self.gram[j0, m + 1 + p] = self.gram[m + 1 + p, j0] = old
        elif self._now("evicted") and full:
            self.slot_of[-1], self.free = self.free, p
        elif self._now("h_diag"):
            self.h_diag = h

    def _recursion(self, lst, k):
        self._first_dot = True
        return super()._recursion(lst, k)

    def _rdot(self, q, lst, row):
        if self._now("lane64") and self._first_dot:
            self._first_dot = False
            return q[lst[:64]] @ self.gram[row, lst[:64]]
        return super()._rdot(q, lst, row)


# ---- the case table.  A case: m, the split of the flat vector into tensors, `null` (indices of tensors whose gradient table
# entry is NULL), lr and the stop rules, and a script of passes (first, gradient, loss):
#   gradient  "quad"         fp32(ev x - b) of the stored parameters (a diagonal quadratic: y = ev s, so ys > 0)
#             ("scale", f)   f times that
#             "repeat"       the previous pass's gradient again (y = 0 exactly)
#             "asif"         fp32(g_prev + ev s) with s the kept pending step: the gradient had that step been taken
#             ("nan", e)     "quad" with element e NaN
#   loss      None = fp32 of the quadratic's value, or a number.
# Condition on every case (asserted by run_case on the reference side, decisions_clear): ys is exactly 0 or >= 1e-6 away from
# 1e-10, and max|g|, max|t d|, |loss - prev_loss| and gtd are a factor >= 2 away from their tolerances.
OFF = dict(max_iter=10 ** 6, max_eval=10 ** 6, tolerance_grad=-1.0, tolerance_change=-1.0)
_SMALL = [1 + (7 * i) % 13 for i in range(68)]
_TABLE = _SMALL[:1] + [3] + _SMALL[1:] + [4097, 5000 - 4097 - sum(_SMALL)]     # 71 tensors, entry 1 has no gradient


def _quad(passes):
    return [(i == 0, "quad", None) for i in range(passes)]


def _case(m, splits, steps, lr=0.25, null=(), x0=2.0, ev_max=4.0, **kw):
    return dict(m=m, splits=list(splits), steps=steps, null=tuple(null), x0=x0, ev_max=ev_max, kw=dict(dict(OFF, lr=lr), **kw))


CASES = {
    # ring
    "ring_m1": _case(1, [1], _quad(6)),                           # empty rotation loop
    "ring_m2": _case(2, [3, 1, 3], _quad(9)),                     # three wraps
    "ring_m5": _case(5, [1025, 1026], _quad(12)),                 # n mod 4 = 3, offsets off a 4-float boundary
    # second trips of the one-wave loops: k passes 32 (L > 64), 64, fills at 70, five wraps; every pair commits
    "trips_m70": _case(70, [1, 299], _quad(76), lr=0.1, x0=10.0, ev_max=30.0),
    "max_history": _case(1024, [64], _quad(6)),
    # 71 tensors (> 64: two launches, a running block base), one of 4097 elements, entry 1 NULL: 72 gather blocks
    "tables": _case(3, _TABLE, _quad(6), null=(1,)),
    "blocks": _case(2, [131072 + 2048 + 1], _quad(5)),            # 66 dot blocks, 131 combine blocks
    # every exit of the scalar pass, m = 3, n = 12
    "exit_first_grad": _case(3, [12], [(True, ("scale", 1e-9), None)], tolerance_grad=1e-7),
    "exit_max_eval": _case(3, [12], _quad(3), max_iter=20, max_eval=3),
    "exit_grad_later": _case(3, [12], _quad(2) + [(False, ("scale", 1e-9), None)], tolerance_grad=1e-7),
    "exit_step_size": _case(3, [12], [(True, "quad", 1.0), (False, "quad", 0.5)], lr=1e-3, tolerance_change=1e-3),
    "exit_loss_change": _case(3, [12], [(True, "quad", 1.0), (False, "quad", 1.0)], tolerance_change=1e-9),
    "exit_max_iter": _case(3, [12], _quad(3), max_iter=3),
    # gtd > -tolerance_change on a first pass (the only break tested there besides the gradient's): s written, parameters
    # kept; the next step()'s first pass commits the pair (kept s, y) and takes the same exit at k = 1
    "exit_gtd": _case(3, [12], [(True, "quad", None), (True, "asif", None)], tolerance_change=1e3),
    "dropped_pair": _case(3, [12], _quad(3) + [(False, "repeat", None), (False, "quad", None)]),
    "two_steps": _case(3, [12], _quad(3) + _quad(3), max_iter=3),
    # one NaN gradient element at k = 0, another at k = 2
    "nan": _case(3, [12], [(True, ("nan", 5), None)] + [(False, "quad", None)] * 3 + [(False, ("nan", 7), None),
                                                                                  (False, "quad", None)]),
}


def problem(case):
    """ev (uniform in [1, ev_max]), b, x0 of the case's diagonal quadratic, from a fixed seed."""
    n = sum(case["splits"])
    rng = np.random.default_rng(1000 + n + case["m"])
    return rng.uniform(1.0, case["ev_max"], n), rng.standard_normal(n), case["x0"] * rng.standard_normal(n)


def n_pad_of(n):
    return (n + 3) & ~3


def split_vecs(vecs, m, n):
    """vecs [(2 (m + 1) + 2), n_pad] fp32 -> S, Y [m + 1, n], gbuf [2, n] as float64 (the layout of include/dsr_hip.h)."""
    v = vecs[:, :n].astype(np.float64)
    return v[:m + 1], v[m + 1:2 * (m + 1)], v[2 * (m + 1):]


class HostBackend:
    """The stored state when no device runs: the driver's own fp32-rounded outputs."""

    def reset(self, case, x0):
        self.m, self.n = case["m"], len(x0)
        self.vecs = np.zeros((2 * (self.m + 1) + 2, n_pad_of(self.n)), dtype=np.float32)
        self.params = x0.copy()
        return self.vecs.copy(), self.params.copy()

    def apply(self, g32, loss32, first, exp):
        m, n = self.m, self.n
        with np.errstate(invalid="ignore"):
            self.vecs[2 * (m + 1) + exp["gcur"], :n] = g32
            self.vecs[m + 1 + exp["p"], :n] = exp["y"].astype(np.float32)
            if exp["mode"] != 0:
                s = exp["s64"].astype(np.float32)
                self.vecs[exp["free"], :n] = s
                if exp["mode"] == 2:
                    self.params = self.params + s
        return self.vecs.copy(), self.params.copy(), list(exp["hdr"]), exp["stop"]


def run_case(case, backend, on_pass=None, driver=PassDriver):
    """Runs the case's script: before each pass the driver is handed the backend's stored state, after it on_pass(i, exp,
    before, after) sees the expectation and both states (vecs, params; after also hdr, stop).  Asserts that no decision
    sits within rounding of its threshold.  Returns the driver."""
    m, n = case["m"], sum(case["splits"])
    ev, b, x0 = problem(case)
    drv = driver(n, history_size=m, **case["kw"])
    null = np.zeros(n, dtype=bool)
    o = 0
    for i, s in enumerate(case["splits"]):
        null[o:o + s] = i in case["null"]
        o += s
    vecs, params = backend.reset(case, x0.astype(np.float32))
    g_last = None
    for i, (first, spec, loss) in enumerate(case["steps"]):
        S, Y, gbuf = split_vecs(vecs, m, n)
        x = np.nan_to_num(params.astype(np.float64), nan=0.0)
        kind, arg = spec if isinstance(spec, tuple) else (spec, None)
        if kind == "repeat":
            g32 = g_last.copy()
        else:
            g = ev * x - b
            if kind == "scale":
                g = arg * g
            elif kind == "asif":
                g = gbuf[drv.gprev] + ev * S[drv.free]
            g32 = g.astype(np.float32)
            if kind == "nan":
                g32[arg] = np.nan
        g32[null] = 0.0
        loss32 = np.float32(0.5 * (ev * x * x).sum() - (b * x).sum() if loss is None else loss)
        with np.errstate(invalid="ignore"):
            exp = drv.expect(S, Y, gbuf, g32.astype(np.float64), float(loss32), first)
        bad = decisions_clear(exp)
        assert not bad, f"pass {i}: decision within rounding of its threshold: {bad}"
        after = backend.apply(g32, loss32, first, exp)
        if on_pass is not None:
            on_pass(i, exp, (vecs, params), after, g32)
        vecs, params, g_last = after[0], after[1], g32
    return drv
