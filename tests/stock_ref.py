"""tests/stock_ref.py -- numpy fp64 restatement of the step of OpenMM's stock integrators as csrc/stock.hip states it (AMM_OP_STOCK).
TEST INFRASTRUCTURE ONLY.

With f the forces at x, m the mass, N a standard normal number per degree of freedom and a = exp(-friction dt):

  0 Verlet          v1 = v + dt f/m ; x' = x + dt v1 ; SHAKE x' along the bond vectors of x ; v = (x' - x)/dt
  1 LangevinMiddle  v1 = v + dt f/m ; RATTLE v1 at x ; xh = x + dt/2 v1 ; v2 = a v1 + sqrt(kT (1 - a^2)/m) N ; x1 = xh + dt/2 v2 ;
                    x' = SHAKE of x1 along the bond vectors of x ; v = v2 + (x' - x1)/dt
  2 Langevin        v1 = a v + b f/m + sqrt(kT (1 - a^2)/m) N, b = (1 - a)/friction (dt when friction = 0) ; then as Verlet
  3 Brownian        x' = x + (dt/friction) f/m + sqrt(2 kT dt/(friction m)) N ; SHAKE ; v = (x' - x)/dt

SHAKE and RATTLE are the Gauss-Seidel sweeps of csrc/cons_sweeps.h in their order: a cluster's constraints in the order they were
given, sweep after sweep until one sweep finds every constraint within the tolerance (at most 500).  Clusters of one pattern are
swept together here (vectorised over the clusters, each with its own stopping sweep): the arithmetic per cluster is the kernel's.
N for step k (k = 1, 2, ... since the seed was set) comes from oracle.expr_oracle.uniforms(3 n, 0, seed, (1 << 63) | k) with
Box-Muller, the stream of AMM_OP_BATH / AMM_OP_EXPR."""
import numpy as np

from oracle import expr_oracle as XO

VERLET, LANGEVIN_MIDDLE, LANGEVIN, BROWNIAN = range(4)
SWEEPS = 500


def gaussians(n, seed, k):
    u1, u2 = XO.uniforms(3 * n, 0, seed, (1 << 63) | k)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)).reshape(n, 3)


class Clusters:
    """The clusters of a constraint set as amm_constraints_create forms them: connected components with at least one constraint,
    numbered by their smallest atom, atoms in increasing order, constraints in the order given; grouped by pattern."""

    def __init__(self, n, pairs, dist):
        parent = list(range(n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for i, j in pairs:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
        atoms, cons = {}, {}
        for i in range(n):
            atoms.setdefault(find(i), []).append(i)
        for q, (i, j) in enumerate(pairs):
            cons.setdefault(find(int(i)), []).append(q)
        self.list = []          # (atoms, local pairs, distances) per cluster
        for root in sorted(cons):
            idx = atoms[root]
            local = [(idx.index(int(pairs[q][0])), idx.index(int(pairs[q][1]))) for q in cons[root]]
            self.list.append((idx, local, [float(dist[q]) for q in cons[root]]))
        batches = {}
        for idx, local, d in self.list:
            batches.setdefault((len(idx), tuple(local)), []).append((idx, d))
        # per pattern: atom indices [nc][na], local pairs, distances [nc][ncons]
        self.batches = [(np.array([idx for idx, _ in members]), list(key[1]), np.array([d for _, d in members]))
                        for key, members in batches.items()]
        self.constrained = np.zeros(n, dtype=bool)
        for idx, _, _ in self.list:
            self.constrained[idx] = True


def _dot3(a, b):
    s = a[:, 0] * b[:, 0]
    s = s + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def _shake_batch(P, R, IM, local, D, tol):
    """P, R: [nc][na][3] positions (changed in place) / reference; IM: [nc][na]; D: [nc][ncons].  Returns sweeps used per cluster
    (SWEEPS + 1: not converged)."""
    lower, upper = 1.0 - 2.0 * tol + tol * tol, 1.0 + 2.0 * tol + tol * tol
    active = np.ones(len(P), dtype=bool)
    used = np.zeros(len(P), dtype=int)
    for _ in range(SWEEPS):
        if not active.any():
            break
        used[active] += 1
        again = np.zeros(len(P), dtype=bool)
        for q, (i, j) in enumerate(local):
            dp, dr = P[:, i] - P[:, j], R[:, i] - R[:, j]
            pp, rp = _dot3(dp, dp), _dot3(dr, dp)
            d2 = D[:, q] * D[:, q]
            hit = active & ~((pp >= lower * d2) & (pp <= upper * d2))       # (negated as in the kernel: NaN also triggers)
            if hit.any():
                g = (d2[hit] - pp[hit]) / (2.0 * (IM[hit, i] + IM[hit, j]) * rp[hit])
                P[hit, i] += (g * IM[hit, i])[:, None] * dr[hit]
                P[hit, j] -= (g * IM[hit, j])[:, None] * dr[hit]
            again |= hit
        active = again
    used[active] = SWEEPS + 1
    return used


def _rattle_batch(P, W, IM, local, tol):
    active = np.ones(len(P), dtype=bool)
    used = np.zeros(len(P), dtype=int)
    for _ in range(SWEEPS):
        if not active.any():
            break
        used[active] += 1
        again = np.zeros(len(P), dtype=bool)
        for i, j in local:
            dp = P[:, i] - P[:, j]
            dot, pp = _dot3(dp, W[:, i] - W[:, j]), _dot3(dp, dp)
            hit = active & ~(np.abs(dot) <= tol * pp)
            if hit.any():
                g = -dot[hit] / ((IM[hit, i] + IM[hit, j]) * pp[hit])
                W[hit, i] += (g * IM[hit, i])[:, None] * dp[hit]
                W[hit, j] -= (g * IM[hit, j])[:, None] * dp[hit]
            again |= hit
        active = again
    used[active] = SWEEPS + 1
    return used


def shake(x, xref, mass, clusters, tol):
    """SHAKE of all clusters; returns (positions, most sweeps any cluster used)."""
    out, worst = x.copy(), 0
    for idx, local, D in clusters.batches:
        P = x[idx]
        used = _shake_batch(P, xref[idx], 1.0 / mass[idx], local, D, tol)
        out[idx] = P
        worst = max(worst, int(used.max()))
    return out, worst


def rattle(x, v, mass, clusters, tol):
    out, worst = v.copy(), 0
    for idx, local, _ in clusters.batches:
        W = v[idx]
        used = _rattle_batch(x[idx], W, 1.0 / mass[idx], local, tol)
        out[idx] = W
        worst = max(worst, int(used.max()))
    return out, worst


def step(kind, x, v, f, mass, clusters, dt, friction, kT, tol, seed, k):
    """One step (the k-th since the seed was set).  clusters: a Clusters, or None for a system without constraints.
    Returns (x', v', most sweeps any solver call used)."""
    n = len(x)
    m = mass[:, None]
    a = np.exp(-friction * dt)
    worst = 0
    N = gaussians(n, seed, k) if kind != VERLET else None
    if kind in (VERLET, LANGEVIN_MIDDLE):
        w = v + (dt * f) / m
    elif kind == LANGEVIN:
        b = (1.0 - a) / friction if friction > 0 else dt
        w = (a * v + (b * f) / m) + np.sqrt((kT * (1.0 - a * a)) / m) * N
    else:
        w = v
    if kind == LANGEVIN_MIDDLE:
        if clusters is not None:
            w, worst = rattle(x, w, mass, clusters, tol)
        xh = x + (0.5 * dt) * w
        w = a * w + np.sqrt((kT * (1.0 - a * a)) / m) * N
        x1 = xh + (0.5 * dt) * w
    elif kind == BROWNIAN:
        x1 = (x + ((dt / friction) * f) / m) + np.sqrt((2.0 * kT * dt / friction) / m) * N
    else:
        x1 = x + dt * w
    xn, sweeps = shake(x1, x, mass, clusters, tol) if clusters is not None else (x1, 0)
    worst = max(worst, sweeps)
    vn = w + (xn - x1) / dt if kind == LANGEVIN_MIDDLE else (xn - x) / dt
    return xn, vn, worst
