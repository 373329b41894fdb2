"""float64 numpy model of the vector-free L-BFGS that csrc/lbfgs.hip implements (Chen, Wang & Zhou, NIPS 2014).

Same state machine as the kernels: m + 1 ring slots, the pending pair (s = t d, y = g - g_prev) kept in the free slot until
the next iteration commits it (ys > 1e-10) or drops it, a Gram matrix over the basis {S slots, Y slots, g} updated only
with the dots of the pending pair and the new gradient, the two-loop recursion on coefficients, and every break of
torch/optim/lbfgs.py decided from scalars.  Only the four passes' arithmetic differs: here dots and combinations are
plain float64 numpy."""
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

    def _pass(self, loss, g, first):
        """gather + dots + scalar + combine for one closure value; returns (stop, update) where update is the
        parameter increment (None when the parameters do not move)."""
        m, nb, G = self.m, self.nb, 2 * (self.m + 1)
        # gather
        gcur = 1 - self.gprev
        p = self.free
        self.gbuf[gcur] = g
        self.Y[p] = g - self.gbuf[self.gprev]
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
        if stop:
            return True, None
        self.n_iter_step += 1
        self.n_iter += 1
        committed = False
        if self.n_iter == 1:
            self.slot_of, self.free, self.h_diag = [], 0, 1.0
        elif pend[1] > 1e-10:
            committed = True
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
        k = len(self.slot_of)
        for j in self.slot_of:
            gs, gy = (pend[3], pend[4]) if committed and j == p else dots[j][4:]
            self.gram[G, j] = self.gram[j, G] = gs
            self.gram[G, m + 1 + j] = self.gram[m + 1 + j, G] = gy
        self.gram[G, G] = pend[5]
        lst = list(self.slot_of) + [m + 1 + j for j in self.slot_of] + [G]
        q = np.zeros(nb)
        q[G] = -1.0
        al = [0.0] * k
        for i in range(k - 1, -1, -1):
            al[i] = (q[lst] @ self.gram[lst[i], lst]) * self.ro[lst[i]]
            q[lst[k + i]] -= al[i]
        q[lst] *= self.h_diag
        for i in range(k):
            be = (q[lst] @ self.gram[lst[k + i], lst]) * self.ro[lst[i]]
            q[lst[i]] += al[i] - be
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
        if gtd > -self.tol_change:
            return True, None
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
