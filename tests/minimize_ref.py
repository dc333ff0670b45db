"""numpy restatement of the minimiser (csrc/minimize.hip + Engine.minimize) -- test infrastructure.

GramLBFGS keeps the ring of pairs (s, y) and the matrix of dot products over b = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g] by ring slot,
and runs the two-loop recursion on that matrix alone, exactly as k_min_coef does: newest pair first, pairs that failed the
curvature test left out, H0 = (s.y / y.y) of the newest pair, steepest descent when g.d >= 0.  `dtype` selects the arithmetic
(np.float64: what the device does up to the order of its sums; np.longdouble: the reference the GPU tests compare with).
two_loop() is the textbook recursion on the vectors themselves; minimize() is the driver Engine.minimize runs (Armijo backtracking,
step cap, restart) over any function x -> (energy, gradient)."""
import math

import numpy as np

CURVATURE = 1e-10
ARMIJO = 1e-4
MAX_HALVINGS = 20


def two_loop(pairs, g):
    """d = -H g by the textbook two-loop recursion; pairs = [(s, y), ...] oldest first."""
    q = np.array(g, dtype=g.dtype)
    alphas = []
    for s, y in reversed(pairs):
        a = np.dot(s, q) / np.dot(s, y)
        alphas.append(a)
        q = q - a * y
    if pairs:
        s, y = pairs[-1]
        q = q * (np.dot(s, y) / np.dot(y, y))
    for (s, y), a in zip(pairs, reversed(alphas)):
        b = np.dot(y, q) / np.dot(s, y)
        q = q + (a - b) * s
    return -q


class GramLBFGS:
    def __init__(self, n3, memory=8, free=None, max_step=0.1, dtype=np.float64):
        self.m, self.n3, self.dtype = memory, n3, dtype
        self.free = np.ones(n3, dtype=bool) if free is None else np.asarray(free, dtype=bool)
        self.max_step = max_step
        self.ring = np.zeros((2 * memory, n3), dtype=dtype)
        self.gram = np.zeros((2 * memory + 1, 2 * memory + 1), dtype=dtype)
        self.valid = [False] * memory
        self.head = 0
        self.dropped = self.resets = self.restarts = 0

    # ---- the three launches of an iteration
    def _basis(self, j):
        return self.gprev if j == 2 * self.m else self.ring[j]

    def _gram_rows(self, rows):
        nb = 2 * self.m + 1
        for r in rows:
            for c in range(nb):
                self.gram[r, c] = self.gram[c, r] = np.dot(self._basis(r), self._basis(c))

    def _coefficients(self, newest, form):
        m, G = self.m, self.gram
        self.newest_dropped = False
        if form:
            sy, ss, yy = G[newest, m + newest], G[newest, newest], G[m + newest, m + newest]
            ok = bool(sy > CURVATURE * np.sqrt(ss * yy))
            self.valid[newest] = ok
            self.newest_dropped = not ok
            self.dropped += 0 if ok else 1
        nb = 2 * m + 1
        in_use = np.array([self.valid[j % m] for j in range(2 * m)] + [True])
        delta = np.zeros(nb, dtype=self.dtype)
        delta[2 * m] = -1

        def dot_row(row):
            return np.dot(np.where(in_use, delta, 0), np.where(in_use, G[row], 0))
        order = [k for k in ((newest - t) % m for t in range(m)) if self.valid[k]]
        alpha = {}
        for k in order:
            alpha[k] = dot_row(k) / G[k, m + k]
            delta[m + k] -= alpha[k]
        if order:
            k = order[0]
            delta *= G[k, m + k] / G[m + k, m + k]
        for k in reversed(order):
            beta = dot_row(m + k) / G[k, m + k]
            delta[k] += alpha[k] - beta
        gd = dot_row(2 * m)
        if not gd < 0:
            delta[:] = 0
            delta[2 * m] = -1
            gd = -G[2 * m, 2 * m]
            self.resets += 1 if order else 0
        self.delta, self.gd, self.in_use = delta, gd, len(order)
        self.gg = G[2 * m, 2 * m]

    def _combine(self):
        d = np.zeros(self.n3, dtype=self.dtype)
        for j in range(2 * self.m + 1):
            if self.delta[j] != 0:
                d = d + self.delta[j] * self._basis(j)
        self.d = d
        self.dmax2 = (d.reshape(-1, 3) ** 2).sum(axis=1).max()

    # ---- the object's entry points (include/atomsmm_hip.h: amm_min_*)
    def begin(self, x, g):
        self.valid = [False] * self.m
        self.head = 0
        self.xprev = np.array(x, dtype=self.dtype)
        self.gprev = np.where(self.free, np.asarray(g, dtype=self.dtype), 0)
        self.gmax = np.abs(self.gprev).max()
        self._gram_rows([2 * self.m])
        self._coefficients(0, False)
        self._combine()

    def restart(self):
        self.valid = [False] * self.m
        self.head = 0
        self.restarts += 1
        self._coefficients(0, False)
        self._combine()

    def advance(self, x, g):
        p, m = self.head, self.m
        x = np.asarray(x, dtype=self.dtype)
        g = np.where(self.free, np.asarray(g, dtype=self.dtype), 0)
        self.ring[p] = np.where(self.free, x - self.xprev, 0)
        self.ring[m + p] = np.where(self.free, g - self.gprev, 0)
        self.xprev, self.gprev = x.copy(), g
        self.gmax = np.abs(g).max()
        self._gram_rows([p, m + p, 2 * m])
        self.head = (p + 1) % m
        self._coefficients(p, True)
        self._combine()

    def step_factor(self, alpha):
        dmax = np.sqrt(self.dmax2)
        return self.max_step / dmax if alpha * dmax > self.max_step else alpha

    def trial(self, alpha):
        a = self.step_factor(alpha)
        if a == 0:
            return self.xprev.copy()
        return np.where(self.free, self.xprev + a * self.d, self.xprev)


def minimize(fun, x0, tolerance=10.0, max_iterations=0, memory=8, max_step=0.1, free=None, reporter=None, dtype=np.float64):
    """Engine.minimize over fun(x) -> (energy, gradient), flat arrays of 3N.  reporter(iteration, x, gradient, energy) -> stop?
    Returns dict(x, energy, iterations, evaluations, reason)."""
    x = np.array(x0, dtype=dtype).ravel()
    lb = GramLBFGS(x.size, memory, free, max_step, dtype)
    nfree = int(lb.free.sum())
    energy, g = fun(x)
    evaluations = 1
    lb.begin(x, g)

    def rms():
        return math.sqrt(float(lb.gg) / nfree)
    iteration, reason = 0, None
    if rms() <= tolerance:
        reason = 'converged'
    alpha = min(1.0, 1.0 / math.sqrt(float(lb.gg))) if lb.gg > 0 else 1.0
    steepest = True
    while reason is None:
        accepted = False
        for _ in range(MAX_HALVINGS + 1):
            a = lb.step_factor(alpha)
            xt = lb.trial(alpha)
            et, gt = fun(xt)
            evaluations += 1
            if math.isfinite(et) and et <= energy + ARMIJO * float(a) * float(lb.gd):
                accepted = True
                break
            alpha = 0.5 * float(a)
        if not accepted:
            if steepest:
                reason = 'no progress'
                break
            lb.restart()
            steepest, alpha = True, 1.0
            continue
        x, energy = xt, et
        stop = bool(reporter(iteration, x, gt, energy)) if reporter is not None else False
        iteration += 1
        if stop:
            reason = 'reporter'
        elif max_iterations and iteration >= max_iterations:
            reason = 'max iterations'
        else:
            lb.advance(x, gt)
            if rms() <= tolerance:
                reason = 'converged'
            steepest, alpha = lb.in_use == 0, 1.0
    return dict(x=np.array(x, dtype=np.float64), energy=float(energy), iterations=iteration, evaluations=evaluations, reason=reason,
                dropped=lb.dropped, restarts=lb.restarts)
