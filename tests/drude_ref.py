"""tests/drude_ref.py -- numpy fp64 restatement of the DrudeForce energy and of the DrudeLangevinIntegrator step as csrc/drude.hip
states them (AMM_FORCE_DRUDE, AMM_OP_DRUDE_STEP).  TEST INFRASTRUCTURE ONLY.

ENERGY (K = 138.935456).  A Drude particle (p, p1, p2, p3, p4, q, alpha, a12, a34): a1 = a12 if p2 != -1 else 1; a2 = a34 if p3 != -1
and p4 != -1 else 1; a3 = 3 - a1 - a2; k3 = K q^2/(alpha a3); k1 = K q^2/(alpha a1) - k3; k2 = K q^2/(alpha a2) - k3; d = x_p - x_p1;
  E = 1/2 k3 |d|^2 + [p2] 1/2 k1 (d.u1)^2 + [p3, p4] 1/2 k2 (d.u2)^2,   u1 = unit(x_p1 - x_p2), u2 = unit(x_p3 - x_p4).
A screened pair (entries A, B, thole t): s = t/(alpha_A alpha_B)^(1/6); sites {p: q, p1: -q} of either entry; per site pair (i, j),
r = |x_i - x_j|, u = s r, S = 1 - (1 + u/2) exp(-u):  E += K q_i q_j S/r,  dE/dr = K q_i q_j (s (1 + u)/2 exp(-u)/r - S/r^2).
Displacements are raw, or each its own minimum image in the orthorhombic box.

`energy_forces` is the analytic gradient; `energy_mp` restates the ENERGY ALONE in mpmath, for the finite differences that check it.

STEP.  a = exp(-gamma dt), b = (1 - a)/gamma (dt when gamma = 0), a_D, b_D from gamma_D; N: one standard normal number per degree of
freedom, an ARGUMENT (stock_ref.gaussians gives the device's stream).  Ordinary massive atom: v1 = a v + b f/m + sqrt(kT (1 - a^2)/m) N.
Pair (Drude p, m1; parent p1, m2; M = m1 + m2; mu = m1 m2/M): v_cm = (m1 v_p + m2 v_p1)/M, v_rel = v_p - v_p1, f_cm = f_p + f_p1,
f_rel = f_p m2/M - f_p1 m1/M; v_cm <- a v_cm + b f_cm/M + sqrt(kT (1 - a^2)/M) N[p1]; v_rel <- a_D v_rel + b_D f_rel/mu +
sqrt(kT_D (1 - a_D^2)/mu) N[p]; v_p = v_cm + v_rel m2/M, v_p1 = v_cm - v_rel m1/M.  Then x' = x + dt v1; SHAKE x' along the bond
vectors of x (stock_ref.shake: the sweeps of cons_sweeps.h); v = (x' - x)/dt; massless particles never move.  Hard wall R > 0, per
pair: d = x_p - x_p1, r = |d|, n = d/r, delta = r - R; r <= R: nothing; r > 2 R: flagged; else w = v.n of both, wbar = (m1 w_p + m2
w_p1)/M subtracted, tau = min(dt, delta/|w_p - w_p1|) (dt if equal), c = sqrt(kT_D/m1), w_p <- -sign(w_p) c m2/M, w_p1 <- -sign(w_p1)
c m1/M, x_p += n (-delta m2/M + tau w_p), x_p1 += n (delta m1/M + tau w_p1), wbar added back.  A massless parent: w_p <- -sign(w_p) c,
x_p += n (-delta + tau w_p), tau = min(dt, delta/|w_p|); such a Drude particle (and the parent of a massless Drude particle) is
thermalised as an ordinary atom."""
import numpy as np

import stock_ref as SR
from atomsmm_amd import unit

KC = 138.935456


def _delta(x, a, b, box):
    d = x[a] - x[b]
    if box is not None:
        d = d - box * np.rint(d / box)
    return d


def spring_constants(row):
    p, p1, p2, p3, p4, q, alpha, a12, a34 = row
    a1 = a12 if p2 != -1 else 1.0
    a2 = a34 if (p3 != -1 and p4 != -1) else 1.0
    a3 = 3.0 - a1 - a2
    k3 = KC * q * q / (alpha * a3)
    return KC * q * q / (alpha * a1) - k3, KC * q * q / (alpha * a2) - k3, k3


def energy_forces(x, rows, pairs, box=None):
    """rows: (p, p1, p2, p3, p4, q, alpha, a12, a34) per Drude particle; pairs: (entry A, entry B, thole); box: edges or None (raw).
    Returns (energy, forces [n][3])."""
    x = np.asarray(x, dtype=np.float64)
    box = None if box is None else np.asarray(box, dtype=np.float64)
    F = np.zeros_like(x)
    E = 0.0
    for row in rows:
        p, p1, p2, p3, p4 = (int(a) for a in row[:5])
        k1, k2, k3 = spring_constants(row)
        d = _delta(x, p, p1, box)
        E += 0.5 * k3 * (d @ d)
        gd = k3 * d
        for k, head, tail, on in ((k1, p1, p2, p2 != -1), (k2, p3, p4, p3 != -1 and p4 != -1)):
            if not on:
                continue
            b = _delta(x, head, tail, box)
            L = np.sqrt(b @ b)
            u = b / L
            s = d @ u
            E += 0.5 * k * s * s
            gd = gd + k * s * u
            gb = k * s * (d - s * u) / L
            F[head] -= gb
            F[tail] += gb
        F[p] -= gd
        F[p1] += gd
    for a, b, thole in pairs:
        ra, rb = rows[int(a)], rows[int(b)]
        s = thole / (ra[6] * rb[6]) ** (1.0 / 6.0)
        for i, qi in ((int(ra[0]), ra[5]), (int(ra[1]), -ra[5])):
            for j, qj in ((int(rb[0]), rb[5]), (int(rb[1]), -rb[5])):
                dv = _delta(x, i, j, box)
                r = np.sqrt(dv @ dv)
                u = s * r
                ex = np.exp(-u)
                S = 1.0 - (1.0 + 0.5 * u) * ex
                kqq = KC * qi * qj
                E += kqq * S / r
                dEdr = kqq * (s * 0.5 * (1.0 + u) * ex / r - S / (r * r))
                g = dEdr * dv / r
                F[i] -= g
                F[j] += g
    return E, F


def energy_mp(x, rows, pairs, box=None):
    """The energy alone in mpmath (x: a list of lists of mpf), term by term from the definition."""
    import mpmath as mp
    K = mp.mpf('138.935456')

    def delta(a, b):
        d = [x[a][c] - x[b][c] for c in range(3)]
        if box is not None:
            d = [d[c] - mp.mpf(box[c]) * mp.nint(d[c] / mp.mpf(box[c])) for c in range(3)]
        return d

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    E = mp.mpf(0)
    for row in rows:
        p, p1, p2, p3, p4 = (int(a) for a in row[:5])
        q, alpha, a12, a34 = (mp.mpf(float(v)) for v in row[5:])
        a1 = a12 if p2 != -1 else mp.mpf(1)
        a2 = a34 if (p3 != -1 and p4 != -1) else mp.mpf(1)
        a3 = 3 - a1 - a2
        k3 = K * q * q / (alpha * a3)
        k1 = K * q * q / (alpha * a1) - k3
        k2 = K * q * q / (alpha * a2) - k3
        d = delta(p, p1)
        E += k3 * dot(d, d) / 2
        if p2 != -1:
            b = delta(p1, p2)
            E += k1 * dot(d, b) ** 2 / dot(b, b) / 2
        if p3 != -1 and p4 != -1:
            b = delta(p3, p4)
            E += k2 * dot(d, b) ** 2 / dot(b, b) / 2
    for a, b, thole in pairs:
        ra, rb = rows[int(a)], rows[int(b)]
        s = mp.mpf(float(thole)) / mp.root(mp.mpf(float(ra[6])) * mp.mpf(float(rb[6])), 6)
        for i, qi in ((int(ra[0]), mp.mpf(float(ra[5]))), (int(ra[1]), -mp.mpf(float(ra[5])))):
            for j, qj in ((int(rb[0]), mp.mpf(float(rb[5]))), (int(rb[1]), -mp.mpf(float(rb[5])))):
                dv = delta(i, j)
                r = mp.sqrt(dot(dv, dv))
                u = s * r
                E += K * qi * qj * (1 - (1 + u / 2) * mp.exp(-u)) / r
    return E


def step(x, v, f, mass, pairs, clusters, dt, friction, kT, drude_friction, drude_kT, wall, tol, N):
    """One step.  pairs: (Drude particle, parent) rows; clusters: a stock_ref.Clusters or None; N: [n][3] standard normal numbers.
    Returns (x', v', flagged, most sweeps a cluster used)."""
    x, v, f, mass = (np.asarray(a, dtype=np.float64) for a in (x, v, f, mass))
    n = len(x)
    a = np.exp(-friction * dt)
    b = (1.0 - a) / friction if friction > 0 else dt
    aD = np.exp(-drude_friction * dt)
    bD = (1.0 - aD) / drude_friction if drude_friction > 0 else dt
    pairs = np.asarray(pairs, dtype=int).reshape(-1, 2)
    both = np.array([mass[p] > 0 and mass[p1] > 0 for p, p1 in pairs], dtype=bool).reshape(-1)
    massive = mass > 0
    safe = np.where(massive, mass, 1.0)[:, None]
    w = v.copy()
    # every massive atom as an ordinary one (the arithmetic of stock_ref.step, kind LANGEVIN); the pairs overwrite theirs
    w[massive] = ((a * v + (b * f) / safe) + np.sqrt((kT * (1.0 - a * a)) / safe) * N)[massive]
    if both.any():
        p, p1 = pairs[both, 0], pairs[both, 1]
        m1, m2 = mass[p][:, None], mass[p1][:, None]
        M = m1 + m2
        mu = m1 * m2 / M
        r2, r1 = m2 / M, m1 / M
        vcm, vrel = (m1 * v[p] + m2 * v[p1]) / M, v[p] - v[p1]
        fcm, frel = f[p] + f[p1], f[p] * r2 - f[p1] * r1
        ncm = (a * vcm + b * fcm / M) + np.sqrt(kT * (1.0 - a * a) / M) * N[p1]
        nrel = (aD * vrel + bD * frel / mu) + np.sqrt(drude_kT * (1.0 - aD * aD) / mu) * N[p]
        w[p] = ncm + nrel * r2
        w[p1] = ncm - nrel * r1
    x1 = x.copy()
    x1[massive] = (x + dt * w)[massive]
    xn, sweeps = SR.shake(x1, x, safe[:, 0], clusters, tol) if clusters is not None else (x1, 0)
    vn = v.copy()
    vn[massive] = ((xn - x) / dt)[massive]
    flagged = False
    if wall > 0:
        for p, p1 in pairs:
            m1, m2 = mass[p], mass[p1]
            if not m1 > 0:
                continue
            d = xn[p] - xn[p1]
            r = np.sqrt(d @ d)
            if r > 2.0 * wall:
                flagged = True
                continue
            if not r > wall:
                continue
            delta = r - wall
            nh = d / r
            wp, w1 = vn[p] @ nh, vn[p1] @ nh
            rp, rq = vn[p] - wp * nh, vn[p1] - w1 * nh
            c = np.sqrt(drude_kT / m1)
            if m2 > 0:
                M = m1 + m2
                f2, f1 = m2 / M, m1 / M
                wbar = (m1 * wp + m2 * w1) / M
                wp, w1 = wp - wbar, w1 - wbar
                gap = abs(wp - w1)
                tau = min(dt, delta / gap) if gap > 0 else dt
                wp = -np.copysign(1.0, wp) * c * f2
                w1 = -np.copysign(1.0, w1) * c * f1
                xn[p] = xn[p] + nh * (-delta * f2 + tau * wp)
                xn[p1] = xn[p1] + nh * (delta * f1 + tau * w1)
                wp, w1 = wp + wbar, w1 + wbar
                vn[p] = rp + wp * nh
                vn[p1] = rq + w1 * nh
            else:
                gap = abs(wp)
                tau = min(dt, delta / gap) if gap > 0 else dt
                wp = -np.copysign(1.0, wp) * c
                xn[p] = xn[p] + nh * (-delta + tau * wp)
                vn[p] = rp + wp * nh
    return xn, vn, flagged, sweeps


def temperatures(v, mass, pairs, n_constraints=0, cm_remover=False, kB=unit.BOLTZMANN_CONSTANT_kB._value):
    """(system temperature, Drude temperature): m v^2 over ordinary massive atoms plus M v_cm^2 over pairs, over dof k_B with dof = 3
    per ordinary massive atom + 3 per pair - constraints - 3 with a CMMotionRemover; m_red v_rel^2 over pairs, over 3 n_pairs k_B."""
    v, mass = np.asarray(v, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=int).reshape(-1, 2)
    ordinary = mass > 0
    ordinary[pairs.reshape(-1)] = False
    p, p1 = pairs[:, 0], pairs[:, 1]
    M = mass[p] + mass[p1]
    mu = mass[p] * mass[p1] / M
    vcm = (mass[p, None] * v[p] + mass[p1, None] * v[p1]) / M[:, None]
    vrel = v[p] - v[p1]
    dof = 3 * int(ordinary.sum()) + 3 * len(pairs) - n_constraints - (3 if cm_remover else 0)
    t_sys = ((mass[ordinary, None] * v[ordinary] ** 2).sum() + (M[:, None] * vcm ** 2).sum()) / (dof * kB)
    t_drude = (mu[:, None] * vrel ** 2).sum() / (3 * len(pairs) * kB)
    return float(t_sys), float(t_drude)
