"""References of the eight bond-list term kinds (test infrastructure; CPU only).

Two independent statements of what include/atomsmm_hip.h says a term's energy is:

  * term_energy_mp / term_forces_mp -- mpmath, 50 digits, from the DEFINITION of each energy.  Angles are atan2(|d1 x d2|, d1 . d2),
    dihedrals the IUPAC angle atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)), every displacement of a periodic kind takes the
    nearest image on its own.  Forces are central differences of that energy at 60 digits with h = 1e-25 nm (the truncation error,
    h^2 E''' / 6, is below 1e-40 of the force at every geometry the tests use, the hard ones included: their smallest length scale is
    1e-9 nm).  Nothing here repeats a term of csrc/bonded_terms.h: no rsqrt, no acos, no 1 - c^2, no Blondel-Karplus gradient.
  * term_np -- plain fp64 numpy, the textbook formulas with their analytic gradients (acos for the angle, the chain rule through
    cos(phi) and sin(phi) for the torsion).  It only serves to MEASURE what an honest fp64 evaluation of these functions loses
    against the reference (tests/bonded_cases.py: TOLERANCE); no GPU result is compared with it.

Kinds and parameters (backend.BOND_* / NPAR; consts: dict(Kc, alpha, rs0, rc0)):
    0 BOND_HARMONIC         (r0, k)            k (r - r0)^2 / 2
    1 ANGLE_HARMONIC        (theta0, k)        k (theta - theta0)^2 / 2, theta at the term's second atom
    2 BOND_LJC              (qq, sigma, eps)   4 eps ((sigma/r)^12 - (sigma/r)^6) + Kc qq / r
    3 BOND_NEAR             (qq, sigma, eps)   S(u) [4 eps ((sigma/r)^12 - (sigma/r)^6 - (sigma/rc0)^12 + (sigma/rc0)^6) + Kc qq (1/r - 1/rc0)],
                                               u = max(0, (r - rs0) / (rc0 - rs0)), S = 1 - 10 u^3 + 15 u^4 - 6 u^5   (the shifted family)
    4 TORSION_PERIODIC      (n, phase, k)      k (1 + cos(n phi - phase))
    5 BOND_EWALD_EXCL       (qq,)              -Kc qq erf(alpha r) / r      (always periodic)
    6 BOND_VIRIAL_HARMONIC  (r0, k)            -k r (r - r0)
    7 BOND_VIRIAL_LJ        (-, sigma, eps)    24 eps (2 (sigma/r)^12 - (sigma/r)^6)
"""
import numpy as np
from mpmath import mp, mpf

ARITY = (2, 3, 2, 2, 4, 2, 2, 2)
NPAR = (2, 2, 3, 3, 3, 1, 2, 3)
KC = 138.935456
CONSTS = dict(Kc=KC, alpha=2.9, rs0=0.4, rc0=0.5)
H_STEP = '1e-25'


# ------------------------------------------------------------------------------------------------------------------- mpmath
def _disp(a, b, box, periodic):
    out = []
    for k in range(3):
        d = a[k] - b[k]
        if periodic:
            L = mpf(float(box[k]))
            d = d - L * mp.nint(d / L)
        out.append(d)
    return out


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def angle_mp(x, box, periodic):
    d1, d2 = _disp(x[0], x[1], box, periodic), _disp(x[2], x[1], box, periodic)
    return mp.atan2(_norm(_cross(d1, d2)), _dot(d1, d2))


def dihedral_mp(x, box, periodic):
    b1, b2, b3 = _disp(x[1], x[0], box, periodic), _disp(x[2], x[1], box, periodic), _disp(x[3], x[2], box, periodic)
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    return mp.atan2(_norm(b2) * _dot(b1, n2), _dot(n1, n2))


def term_energy_mp(kind, x, p, periodic, box, consts=CONSTS):
    """x: the term's atoms as lists of three mpf; p: the parameters (floats, taken exactly)."""
    p = [mpf(float(v)) for v in p]
    if kind == 1:
        return p[1] * (angle_mp(x, box, periodic) - p[0]) ** 2 / 2
    if kind == 4:
        return p[2] * (1 + mp.cos(p[0] * dihedral_mp(x, box, periodic) - p[1]))
    r = _norm(_disp(x[0], x[1], box, periodic or kind == 5))
    Kc = mpf(float(consts['Kc']))
    if kind == 0:
        return p[1] * (r - p[0]) ** 2 / 2
    if kind == 2:
        s6 = (p[1] / r) ** 6
        return 4 * p[2] * (s6 * s6 - s6) + Kc * p[0] / r
    if kind == 3:
        rs0, rc0 = mpf(float(consts['rs0'])), mpf(float(consts['rc0']))
        u = (r - rs0) / (rc0 - rs0)
        u = u if u > 0 else mpf(0)
        S = 1 - 10 * u ** 3 + 15 * u ** 4 - 6 * u ** 5
        s6, c6 = (p[1] / r) ** 6, (p[1] / rc0) ** 6
        return S * (4 * p[2] * (s6 * s6 - s6 - c6 * c6 + c6) + Kc * p[0] * (1 / r - 1 / rc0))
    if kind == 5:
        return -Kc * p[0] * mp.erf(mpf(float(consts['alpha'])) * r) / r
    if kind == 6:
        return -p[1] * r * (r - p[0])
    if kind == 7:
        s6 = (p[1] / r) ** 6
        return 24 * p[2] * (2 * s6 * s6 - s6)
    raise ValueError(kind)


def term_forces_mp(kind, xyz, p, periodic, box, consts=CONSTS):
    """(energy, forces[arity][3]) as mpf: central differences of term_energy_mp at 60 digits.  xyz: [arity][3] floats."""
    old = mp.dps
    mp.dps = 60
    try:
        h = mpf(H_STEP)
        x = [[mpf(float(v)) for v in row] for row in xyz]
        e = term_energy_mp(kind, x, p, periodic, box, consts)
        f = []
        for a in range(len(x)):
            row = []
            for k in range(3):
                keep = x[a][k]
                x[a][k] = keep + h
                ep = term_energy_mp(kind, x, p, periodic, box, consts)
                x[a][k] = keep - h
                em = term_energy_mp(kind, x, p, periodic, box, consts)
                x[a][k] = keep
                row.append(-(ep - em) / (2 * h))
            f.append(row)
        return e, f
    finally:
        mp.dps = old


class Reference:
    """Per-term energies and forces of a case (bonded_cases.Case) from the mpmath reference, rounded to fp64 at the very end.
    e_terms[t], f_terms[t][role][3] (unused roles zero), and the per-atom sums with their units S_i = sum |F_t,i|."""

    def __init__(self, case, consts=CONSTS):
        nt = len(case.terms)
        self.e_terms = np.zeros(nt)
        self.f_terms = np.zeros((nt, 4, 3))
        f_sum = [[mpf(0)] * 3 for _ in range(case.n)]
        e_sum = mpf(0)
        mp.dps = 60
        for t, (kind, atoms, par) in enumerate(case.terms):
            e, f = term_forces_mp(kind, case.x[list(atoms)], par, case.periodic[kind], case.box, consts)
            mp.dps = 60
            e_sum += e
            self.e_terms[t] = float(e)
            for r, a in enumerate(atoms):
                for k in range(3):
                    self.f_terms[t, r, k] = float(f[r][k])
                    f_sum[a][k] += f[r][k]
        mp.dps = 50
        self.energy = float(e_sum)
        self.forces = np.array([[float(v) for v in row] for row in f_sum]).reshape(case.n, 3)
        self.e_unit = float(np.abs(self.e_terms).sum())
        self.kinds = np.array([k for k, _, _ in case.terms], dtype=int)

    def units(self, case, kind=None):
        """S_i = sum over the terms at atom i (of `kind`, or of all kinds) of |F_t,i| (Euclidean norm): the unit of a force error"""
        out = np.zeros(case.n)
        for t, (k, atoms, _) in enumerate(case.terms):
            if kind is None or k == kind:
                for r, a in enumerate(atoms):
                    out[a] += np.linalg.norm(self.f_terms[t, r])
        return out

    def permuted(self, perm):
        """the reference of the same system with atom i renumbered perm[i] (terms keep their order)"""
        import copy
        out = copy.copy(self)
        out.forces = np.empty_like(self.forces)
        out.forces[perm] = self.forces
        return out


# ------------------------------------------------------------------------------------------------------------------- numpy fp64
def _disp_np(a, b, box, periodic):
    d = a - b
    return d - box * np.rint(d / box) if periodic else d


def term_np(kind, xyz, p, periodic, box, consts=CONSTS):
    """(energy, forces[arity][3]) in plain fp64 from the textbook formulas."""
    from math import acos, cos, erf, exp, pi, sin, sqrt
    x = np.asarray(xyz, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    if kind == 1:
        d1, d2 = _disp_np(x[0], x[1], box, periodic), _disp_np(x[2], x[1], box, periodic)
        r1, r2 = sqrt(d1 @ d1), sqrt(d2 @ d2)
        c = max(-1.0, min(1.0, (d1 @ d2) / (r1 * r2)))
        th = acos(c)
        s = sqrt(1.0 - c * c)
        dE = p[1] * (th - p[0])
        fi = dE / s * (d2 / r2 - c * d1 / r1) / r1           # -dE/dtheta dtheta/dx_i, dtheta/dcos = -1/sin
        fk = dE / s * (d1 / r1 - c * d2 / r2) / r2
        return 0.5 * p[1] * (th - p[0]) ** 2, np.array([fi, -(fi + fk), fk])
    if kind == 4:
        b1, b2, b3 = _disp_np(x[1], x[0], box, periodic), _disp_np(x[2], x[1], box, periodic), _disp_np(x[3], x[2], box, periodic)
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        lb2 = sqrt(b2 @ b2)
        phi = np.arctan2(lb2 * (b1 @ n2), n1 @ n2)
        dE = -p[2] * p[0] * sin(p[0] * phi - p[1])
        # Bekker's gradient of the dihedral angle
        g0 = -lb2 / (n1 @ n1) * n1
        g3 = lb2 / (n2 @ n2) * n2
        s12, s32 = (b1 @ b2) / (b2 @ b2), (b3 @ b2) / (b2 @ b2)
        g1 = -g0 - s12 * g0 + s32 * g3
        g2 = -g3 + s12 * g0 - s32 * g3
        return p[2] * (1.0 + cos(p[0] * phi - p[1])), -dE * np.array([g0, g1, g2, g3])
    d = _disp_np(x[0], x[1], box, periodic or kind == 5)
    r = sqrt(d @ d)
    Kc = consts['Kc']
    if kind == 0:
        e, dE = 0.5 * p[1] * (r - p[0]) ** 2, p[1] * (r - p[0])
    elif kind == 2:
        s6 = (p[1] / r) ** 6
        e = 4 * p[2] * (s6 * s6 - s6) + Kc * p[0] / r
        dE = 4 * p[2] * (-12 * s6 * s6 + 6 * s6) / r - Kc * p[0] / (r * r)
    elif kind == 3:
        rs0, rc0 = consts['rs0'], consts['rc0']
        u = max(0.0, (r - rs0) / (rc0 - rs0))
        S = 1 - 10 * u ** 3 + 15 * u ** 4 - 6 * u ** 5
        dS = -30 * u * u * (1 - u) ** 2 / (rc0 - rs0)
        s6, c6 = (p[1] / r) ** 6, (p[1] / rc0) ** 6
        V = 4 * p[2] * (s6 * s6 - s6 - c6 * c6 + c6) + Kc * p[0] * (1 / r - 1 / rc0)
        dV = 4 * p[2] * (-12 * s6 * s6 + 6 * s6) / r - Kc * p[0] / (r * r)
        e, dE = S * V, S * dV + dS * V
    elif kind == 5:
        a = consts['alpha']
        e = -Kc * p[0] * erf(a * r) / r
        dE = -Kc * p[0] * (2 * a / sqrt(pi) * exp(-a * a * r * r) / r - erf(a * r) / (r * r))
    elif kind == 6:
        e, dE = -p[1] * r * (r - p[0]), -p[1] * (2 * r - p[0])
    elif kind == 7:
        s6 = (p[1] / r) ** 6
        e, dE = 24 * p[2] * (2 * s6 * s6 - s6), 24 * p[2] * (-24 * s6 * s6 + 6 * s6) / r
    else:
        raise ValueError(kind)
    f = -dE * d / r
    return e, np.array([f, -f])
