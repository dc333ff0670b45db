"""Host side of the tabulated functions of a CustomNonbondedForce (openmm.Continuous1DFunction, Discrete1DFunction,
Discrete2DFunction) on the pair-expression kernel (csrc/pair_expr.hip): the spline solve, the data the device reads,
the same functions as host callables (the symmetry checks of translate/ evaluate the text with them), and the check of the
per-particle values that a text passes straight into a discrete function.

A Continuous1DFunction is the natural cubic spline (second derivative 0 at both ends) through its values at equally spaced knots
min .. max, and 0 outside [min, max].  It is solved HERE, once, in fp64 -- a tridiagonal (Thomas) solve for the knots' second
derivatives M -- and uploaded as four polynomial coefficients per interval,

    S(t) = a + u (b + u (c + u d)),  u = t - knot_k,   a = y_k,  b = (y_k+1 - y_k)/h - h (2 M_k + M_k+1)/6,  c = M_k/2,
                                                        d = (M_k+1 - M_k)/(6 h)

so that the device gets value and derivative from ONE 32-byte record and two Horner chains (DESIGN.md 3.PT says why not knot values
plus second derivatives).
"""
import ast

import numpy as np

from . import expr as X

CONTINUOUS1D, DISCRETE1D, DISCRETE2D = 0, 1, 2          # AMM_TABLE_* (include/atomsmm_hip.h)
KIND_NAMES = {CONTINUOUS1D: 'Continuous1D', DISCRETE1D: 'Discrete1D', DISCRETE2D: 'Discrete2D'}          # keys of expr.TABLE_KINDS


def spline_second_derivatives(values, lo, hi):
    """M[k] = S''(knot k) of the natural cubic spline through `values` at len(values) equally spaced knots lo .. hi: M[0] = M[-1] = 0,
    M[k-1] + 4 M[k] + M[k+1] = 6 (y[k-1] - 2 y[k] + y[k+1]) / h^2 inside, by forward elimination and back substitution."""
    y = np.asarray(values, dtype=np.float64).reshape(-1)
    n = len(y)
    h = (float(hi) - float(lo)) / (n - 1)
    m = np.zeros(n)
    if n < 3:
        return m
    rhs = 6.0 * (y[:-2] - 2.0 * y[1:-1] + y[2:]) / (h * h)
    k = n - 2
    diag, out = np.empty(k), np.empty(k)
    diag[0], out[0] = 4.0, rhs[0]
    for i in range(1, k):
        w = 1.0 / diag[i - 1]
        diag[i] = 4.0 - w
        out[i] = rhs[i] - w * out[i - 1]
    m[k] = out[k - 1] / diag[k - 1]
    for i in range(k - 2, -1, -1):
        m[i + 1] = (out[i] - m[i + 2]) / diag[i]
    return m


def spline_coefficients(values, lo, hi):
    """[len(values) - 1][4] coefficients (a, b, c, d) of the intervals' cubics in u = t - left knot."""
    y = np.asarray(values, dtype=np.float64).reshape(-1)
    n = len(y)
    h = (float(hi) - float(lo)) / (n - 1)
    m = spline_second_derivatives(y, lo, hi)
    coef = np.empty((n - 1, 4))
    coef[:, 0] = y[:-1]
    coef[:, 1] = (y[1:] - y[:-1]) / h - h * (2.0 * m[:-1] + m[1:]) / 6.0
    coef[:, 2] = 0.5 * m[:-1]
    coef[:, 3] = (m[1:] - m[:-1]) / (6.0 * h)
    return coef


def spline_eval(coef, lo, hi, t):
    """(S(t), S'(t)) as pexpr_table of csrc/pair_expr_vm.h takes them, operation by operation: 0 outside [lo, hi], the interval
    min(floor((t - lo) / h), n - 2), u = (t - lo) - k h, Horner.  t: a number or an array."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 4)
    nx = len(coef) + 1
    t = np.asarray(t, dtype=np.float64)
    h = (float(hi) - float(lo)) / (nx - 1)
    inv_h = (nx - 1) / (float(hi) - float(lo))
    with np.errstate(invalid='ignore'):
        outside = (t < lo) | (t > hi)
        s = (t - lo) * inv_h
        k = np.where((s >= 0.0) & (s < nx), s, 0.0).astype(np.int64)
    k = np.clip(k, 0, nx - 2)
    u = (t - lo) - k * h
    a, b, c, d = coef[k, 0], coef[k, 1], coef[k, 2], coef[k, 3]
    value = a + u * (b + u * (c + u * d))
    slope = b + u * (2.0 * c + u * (3.0 * d))
    return np.where(outside, 0.0, value), np.where(outside, 0.0, slope)


def _periodic_node_slopes(y):
    """dS/du at the nodes of the periodic cubic spline through y along axis 0, in units of the node spacing (u = node index):
    d[k-1] + 4 d[k] + d[k+1] = 3 (y[k+1] - y[k-1]) with the indices taken modulo len(y).  The cyclic system is solved directly (the
    sizes are tens); with two nodes both neighbours are the other node and the slopes come out 0."""
    n = y.shape[0]
    a = np.zeros((n, n))
    for k in range(n):
        a[k, k] += 4.0
        a[k, (k - 1) % n] += 1.0
        a[k, (k + 1) % n] += 1.0
    return np.linalg.solve(a, 3.0 * (np.roll(y, -1, axis=0) - np.roll(y, 1, axis=0)))


# cubic Hermite basis in monomial form: (p(0), p(1), p'(0), p'(1)) -> the coefficients of 1, u, u^2, u^3
_HERMITE = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [-3.0, 3.0, -2.0, -1.0], [2.0, -2.0, 1.0, 1.0]])


def cmap_coefficients(size, energy):
    """The map of a CMAPTorsionForce as the device reads it (csrc/cmap.hip): [size * size][16] coefficients, row
    s + size * t for the cell phi in [s, s + 1) delta, psi in [t, t + 1) delta (delta = 2 pi / size), with

        E = sum_ij c[4 i + j] da^i db^j,   da, db in [0, 1) the fractional positions of phi and psi within the cell.

    energy[i + size * j] is the value at phi = i delta, psi = j delta.  The interpolant is the tensor-product periodic cubic spline
    through the map (what OpenMM's CMAPTorsionForceImpl builds): dE/dphi at the nodes from the periodic spline through every row,
    dE/dpsi from every column, d2E/dphi dpsi from the periodic spline through the dE/dphi values along psi; a cell's patch matches
    the four quantities at its four corners.  Derivatives are in cell units here: the kernel divides by delta."""
    size = int(size)
    y = np.asarray(energy, dtype=np.float64).reshape(-1)
    if size < 2 or len(y) != size * size:
        raise ValueError('a CMAP map of size %d needs %d values, and a size of at least 2' % (size, size * size))
    f = y.reshape(size, size).T                     # f[i, j]: phi index i, psi index j
    fx = _periodic_node_slopes(f)                   # along phi
    fy = _periodic_node_slopes(f.T).T               # along psi
    fxy = _periodic_node_slopes(fx.T).T             # dE/dphi, splined along psi
    nxt = np.arange(1, size + 1) % size
    corner = np.empty((size, size, 4, 4))           # [s, t][(f | d/dphi) at s, s + 1][(f | d/dpsi) at t, t + 1]
    for a, rows in enumerate((np.arange(size), nxt)):
        for b, cols in enumerate((np.arange(size), nxt)):
            corner[:, :, a, b] = f[np.ix_(rows, cols)]
            corner[:, :, 2 + a, b] = fx[np.ix_(rows, cols)]
            corner[:, :, a, 2 + b] = fy[np.ix_(rows, cols)]
            corner[:, :, 2 + a, 2 + b] = fxy[np.ix_(rows, cols)]
    c = np.einsum('ia,stab,jb->stij', _HERMITE, corner, _HERMITE)
    return np.ascontiguousarray(c.transpose(1, 0, 2, 3).reshape(size * size, 16))


def cmap_eval(coef, size, phi, psi):
    """(E, dE/dphi, dE/dpsi) at angles in radians as k_cmap of csrc/cmap.hip takes them, operation by operation: the angle brought to
    [0, 2 pi), u = angle / delta, the cell (int)u reduced modulo size, nested Horner.  phi, psi: numbers or arrays."""
    coef = np.asarray(coef, dtype=np.float64).reshape(size * size, 16)
    delta = 2.0 * np.pi / size

    def cell(angle):
        angle = np.asarray(angle, dtype=np.float64)
        u = np.where(angle < 0.0, angle + 2.0 * np.pi, angle) / delta
        s = u.astype(np.int64)
        return s % size, u - s

    (s, da), (t, db) = cell(phi), cell(psi)
    c = coef[s + size * t]
    r = [((c[..., 4 * i + 3] * db + c[..., 4 * i + 2]) * db + c[..., 4 * i + 1]) * db + c[..., 4 * i] for i in range(4)]
    d = [(3.0 * c[..., 4 * i + 3] * db + 2.0 * c[..., 4 * i + 2]) * db + c[..., 4 * i + 1] for i in range(4)]
    e = ((r[3] * da + r[2]) * da + r[1]) * da + r[0]
    de_da = (3.0 * r[3] * da + 2.0 * r[2]) * da + r[1]
    de_db = ((d[3] * da + d[2]) * da + d[1]) * da + d[0]
    return e, de_da / delta, de_db / delta


def kind_of(function):
    """AMM_TABLE_* of an openmm tabulated-function object."""
    return function._amm_table_kind


def declared(functions):
    """The `functions` argument of expr.compile_pair for [(name, function)] in the force's order."""
    return {name: (KIND_NAMES[kind_of(fn)], 2 if kind_of(fn) == DISCRETE2D else 1) for name, fn in functions}


def device_table(function):
    """(kind, nx, ny, lo, hi, doubles) of one function: what amm_pair_expr_set_tables takes for it."""
    kind = kind_of(function)
    if kind == CONTINUOUS1D:
        values, lo, hi = function.getFunctionParameters()
        return kind, len(values), 1, float(lo), float(hi), spline_coefficients(values, lo, hi).reshape(-1)
    if kind == DISCRETE1D:
        values = np.asarray(function.getFunctionParameters(), dtype=np.float64).reshape(-1)
        return kind, len(values), 1, 0.0, 0.0, values
    xsize, ysize, values = function.getFunctionParameters()
    return kind, int(xsize), int(ysize), 0.0, 0.0, np.asarray(values, dtype=np.float64).reshape(-1)


def host_callable(function):
    """The function as the kernel evaluates it, on numbers: the spline (0 outside its range); values[rint(x)], NaN for an index that is
    NaN or outside the table."""
    kind, nx, ny, lo, hi, data = device_table(function)
    if kind == CONTINUOUS1D:
        return lambda t: float(spline_eval(data, lo, hi, float(t))[0])

    def lookup(x, y=0.0):
        rx, ry = np.rint(x), np.rint(y)
        if not (0.0 <= rx < nx and 0.0 <= ry < ny):
            return float('nan')
        return float(data[int(rx) + nx * int(ry)])
    return lookup


def direct_index_uses(text, functions):
    """Where a symbol is passed DIRECTLY as an argument of a discrete function -- f(type1), g(type1, type2): [(symbol, function name,
    size of the table along that argument)].  An index computed by arithmetic is not listed (the kernel's NaN rule covers it)."""
    sizes = {}
    for name, fn in functions:
        kind = kind_of(fn)
        if kind == DISCRETE1D:
            sizes[name] = (len(fn.getFunctionParameters()),)
        elif kind == DISCRETE2D:
            sizes[name] = tuple(int(s) for s in fn.getFunctionParameters()[:2])
    main, defs = X.split_definitions(text)
    found = []
    for part in [main] + list(defs.values()):
        for node in ast.walk(X._parse(part)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in sizes and len(node.args) == len(sizes[node.func.id]):
                for arg, size in zip(node.args, sizes[node.func.id]):
                    if isinstance(arg, ast.Name) and (arg.id, node.func.id, size) not in found:
                        found.append((arg.id, node.func.id, size))
    return found
