"""TEST INFRASTRUCTURE (checker only) of the tabulated functions of a CustomNonbondedForce (atomsmm_amd/tables.py, csrc/pair_expr_vm.h:
pexpr_table): the reference spline and a reference pair sum.  Nothing here shares code with atomsmm_amd.

Reference spline: scipy.interpolate.CubicSpline(knots, values, bc_type='natural') and its .derivative() -- the SPECIFICATION of a
Continuous1DFunction inside [min, max]; outside, value and derivative are 0.
Reference sum: a fp64 O(N^2) minimum-image sum over the pairs that are not excluded and have r < rc (pair_expr_cases.pairs_within),
the radial function given in closed form by numpy; OpenMM's built-in switch in closed form (pair_expr_cases.switch).
"""
import numpy as np
from scipy.interpolate import CubicSpline

import pair_expr_cases as P


def reference_spline(values, lo, hi):
    """(S, S') as callables on arrays: the natural cubic spline through `values` at equally spaced knots lo .. hi, 0 outside."""
    knots = np.linspace(lo, hi, len(values))
    spline = CubicSpline(knots, np.asarray(values, dtype=np.float64), bc_type='natural')
    slope = spline.derivative()

    def inside(t):
        t = np.asarray(t, dtype=np.float64)
        return (t >= lo) & (t <= hi)
    return (lambda t: np.where(inside(t), spline(t), 0.0)), (lambda t: np.where(inside(t), slope(t), 0.0))


def tabulated_u(lo, hi, knots=901):
    """The values of U(r) = 1e5 exp(-30 r) - 3e-3 / r^6 at `knots` equally spaced radii lo .. hi."""
    r = np.linspace(lo, hi, knots)
    return 1e5 * np.exp(-30.0 * r) - 3e-3 / r ** 6


def radial_sum(radial, positions, box, rc, excl_pairs=(), rswitch=None, r_from=None):
    """(energy, forces [n][3], pairs counted): sum over the pairs i < j that are not excluded and have r < rc (and r >= r_from) of
    E(i, j, r), with (E, dE/dr) = radial(i, j, r) on arrays."""
    n = len(positions)
    i, j, r, d = P.pairs_within(positions, box, rc, excl_pairs)
    if r_from is not None:
        keep = r >= r_from
        i, j, r, d = i[keep], j[keep], r[keep], d[keep]
    e, de = radial(i, j, r)
    if rswitch is not None:
        s, ds = P.switch(r, rswitch, rc)
        e, de = s * e, s * de + ds * e
    f = (-de / r)[:, None] * d
    forces = np.zeros((n, 3))
    np.add.at(forces, i, f)
    np.add.at(forces, j, -f)
    return float(e.sum()), forces, len(r)


def types_by_mass(mass):
    """(type index per atom, number of types): atoms of equal rounded mass share a type, in order of mass."""
    _, kind = np.unique(np.rint(np.asarray(mass, dtype=np.float64)), return_inverse=True)
    kind = kind.reshape(-1)
    return kind, int(kind.max()) + 1


def buckingham_tables(mass, seed=P.SEED):
    """The type-pair matrices A, B, C [types][types] that pair_expr_cases.TEXTS['buckingham']'s mixing rules give at its seeded
    per-type draws, the atoms' types, and the per-atom (A, B, C) rows of the mixing-rule text."""
    case = P.TEXTS['buckingham']
    kind, ntypes = types_by_mass(mass)
    rows = P.typed_parameters(case, np.rint(mass), seed)
    per_type = np.array([rows[np.nonzero(kind == t)[0][0]] for t in range(ntypes)])
    a, b, c = per_type[:, 0], per_type[:, 1], per_type[:, 2]
    return kind, rows, np.sqrt(np.outer(a, a)), 0.5 * (b[:, None] + b[None, :]), np.sqrt(np.outer(c, c))


def buckingham_radial(kind, A, B, C):
    """radial(i, j, r) of A(ti,tj) exp(-B(ti,tj) r) - C(ti,tj) / r^6 in closed form."""
    def radial(i, j, r):
        a, b, c = A[kind[i], kind[j]], B[kind[i], kind[j]], C[kind[i], kind[j]]
        ex = a * np.exp(-b * r)
        return ex - c / r ** 6, -b * ex + 6.0 * c / r ** 7
    return radial
