"""TEST INFRASTRUCTURE (checker only) of the term-expression forces (csrc/term_expr.hip): texts, a reference sum over terms and a
plain-Python restatement of the interpreter's term leaves.

Reference: per term, the geometric variable -- r, the angle theta in [0, pi], the dihedral theta in (-pi, pi] with the sign convention
of PeriodicTorsionForce, or the raw x, y, z -- is computed from the atoms' coordinates in mpmath at 50 digits, the energy is the TEXT
evaluated by tests/expr_reference.py at that value, and every force component is -mpmath.diff of that energy in the Cartesian
coordinate itself.  The reference therefore shares neither the compiler nor the interpreter nor the analytic gradients of the kernels.

Inputs to avoid (`usable`): angles within 1e-3 of 0 or pi, torsions with a (nearly) collinear triple, and the kinks of min / max / abs
that a text declares (`kinks`: quantities that must stay away from zero).  expr_reference.Unstable reports select / step / floor.
"""
import math

import mpmath
import numpy as np

import expr_reference as R
import pair_expr_cases as P
from atomsmm_amd import expr as X

BOND, ANGLE, TORSION, EXTERNAL = range(4)
VARIABLES = {BOND: ('r',), ANGLE: ('theta',), TORSION: ('theta',), EXTERNAL: ('x', 'y', 'z')}
ARITY = {BOND: 2, ANGLE: 3, TORSION: 4, EXTERNAL: 1}
PI_TEXT = 'pi = 3.141592653589793'
KINK_MARGIN = 1e-3

# name -> kind, text, per-term parameter names, globals, kinks(variables, parameters, globals) -> quantities that must not be near 0
TEXTS = {
    'harmonic-bond': dict(kind=BOND, text='0.5*k*(r-r0)^2', names=['r0', 'k'], globals={}, kinks=lambda v, p, g: []),
    'harmonic-angle': dict(kind=ANGLE, text='0.5*k*(theta-theta0)^2', names=['theta0', 'k'], globals={}, kinks=lambda v, p, g: []),
    'periodic-torsion': dict(kind=TORSION, text='k*(1+cos(n*theta-theta0))', names=['n', 'theta0', 'k'], globals={},
                             kinks=lambda v, p, g: []),
    'morse': dict(kind=BOND, text='D*(1-exp(-a*(r-r0)))^2', names=['D', 'a', 'r0'], globals={}, kinks=lambda v, p, g: []),
    'morse-global': dict(kind=BOND, text='scale*D*(1-exp(-a*(r-r0)))^2', names=['D', 'r0'], globals=dict(scale=1.5, a=12.0),
                         kinks=lambda v, p, g: []),
    'fene': dict(kind=BOND, text='-0.5*k*R0^2*log(1-(r/R0)^2)', names=['k', 'R0'], globals={}, kinks=lambda v, p, g: []),
    'cosine-angle': dict(kind=ANGLE, text='0.5*k*(cos(theta)-cos(theta0))^2', names=['theta0', 'k'], globals={},
                         kinks=lambda v, p, g: []),
    'rb-torsion': dict(kind=TORSION, text='c0+c1*cp+c2*cp^2+c3*cp^3+c4*cp^4+c5*cp^5; cp=cos(psi); psi=theta-pi; ' + PI_TEXT,
                       names=['c0', 'c1', 'c2', 'c3', 'c4', 'c5'], globals={}, kinks=lambda v, p, g: []),
    'charmm-improper': dict(kind=TORSION, text='k*min(dtheta, 2*pi-dtheta)^2; dtheta = abs(theta-theta0); ' + PI_TEXT,
                            names=['k', 'theta0'], globals={},
                            kinks=lambda v, p, g: [v[0] - p[1], math.pi - abs(v[0] - p[1])]),
    'position-restraint': dict(kind=EXTERNAL, text='0.5*k*((x-x0)^2+(y-y0)^2+(z-z0)^2)', names=['k', 'x0', 'y0', 'z0'], globals={},
                               kinks=lambda v, p, g: []),
    'flat-bottom': dict(kind=EXTERNAL, text='k*max(0, d-d0)^2; d = sqrt((x-x0)^2+(y-y0)^2+(z-z0)^2)', names=['k', 'd0', 'x0', 'y0', 'z0'],
                        globals={}, kinks=lambda v, p, g: [math.dist(v, p[2:5]) - p[1]]),
    'wall': dict(kind=EXTERNAL, text='kw*step(z-zw)*(z-zw)^4 + g*m*z', names=['m'], globals=dict(kw=50.0, zw=1.2, g=0.3),
                 kinks=lambda v, p, g: [v[2] - g['zw']]),
}


# ------------------------------------------------------------------------------------------------ geometry, fp64 (selection only)
def displacement(a, b, box=None):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    if box is not None:
        d = d - np.asarray(box) * np.rint(d / np.asarray(box))
    return d


def variables_of(kind, pos, atoms, box=None):
    """The term's variables in fp64 (for choosing inputs and for closed forms, never as the reference of a comparison)."""
    x = [np.asarray(pos[a], dtype=np.float64) for a in atoms[:ARITY[kind]]]
    if kind == EXTERNAL:
        return tuple(float(c) for c in x[0])
    if kind == BOND:
        return (float(np.linalg.norm(displacement(x[0], x[1], box))),)
    if kind == ANGLE:
        d1, d2 = displacement(x[0], x[1], box), displacement(x[2], x[1], box)
        return (float(math.acos(max(-1.0, min(1.0, d1.dot(d2) / math.sqrt(d1.dot(d1) * d2.dot(d2)))))),)
    F, G, H = displacement(x[0], x[1], box), displacement(x[1], x[2], box), displacement(x[3], x[2], box)
    A, Bv = np.cross(F, G), np.cross(H, G)
    return (float(math.atan2(np.cross(Bv, A).dot(G) / math.sqrt(G.dot(G)), A.dot(Bv))),)


def usable(case, pos, atoms, params, box=None, gvalues=None):
    """True when the term is none of the inputs to avoid."""
    kind = case['kind']
    v = variables_of(kind, pos, atoms, box)
    if kind == ANGLE and not (KINK_MARGIN < v[0] < math.pi - KINK_MARGIN):
        return False
    if kind == TORSION:
        x = [np.asarray(pos[a], dtype=np.float64) for a in atoms[:4]]
        for i, j, k in ((0, 1, 2), (1, 2, 3)):
            d1, d2 = displacement(x[i], x[j], box), displacement(x[k], x[j], box)
            s = np.linalg.norm(np.cross(d1, d2)) / math.sqrt(d1.dot(d1) * d2.dot(d2))
            if s < 0.05:
                return False
        if abs(abs(v[0]) - math.pi) < KINK_MARGIN:          # the cut of atan2: theta jumps by 2 pi
            return False
    g = dict(case['globals'] if gvalues is None else gvalues)
    return all(abs(q) > KINK_MARGIN for q in case['kinks'](v, list(params), g))


# ------------------------------------------------------------------------------------------------ the reference, mpmath
def _mp_variables(kind, coords, box):
    """The term's variables from 3 * arity mpf coordinates."""
    x = [coords[3 * a:3 * a + 3] for a in range(len(coords) // 3)]

    def delta(a, b):
        d = [p - q for p, q in zip(x[a], x[b])]
        if box is not None:
            d = [c - mpmath.mpf(float(L)) * mpmath.nint(c / mpmath.mpf(float(L))) for c, L in zip(d, box)]
        return d

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    if kind == EXTERNAL:
        return dict(x=x[0][0], y=x[0][1], z=x[0][2])
    if kind == BOND:
        d = delta(0, 1)
        return dict(r=mpmath.sqrt(dot(d, d)))
    if kind == ANGLE:
        d1, d2 = delta(0, 1), delta(2, 1)
        return dict(theta=mpmath.acos(dot(d1, d2) / mpmath.sqrt(dot(d1, d1) * dot(d2, d2))))
    F, G, H = delta(0, 1), delta(1, 2), delta(3, 2)
    A, Bv = cross(F, G), cross(H, G)
    return dict(theta=mpmath.atan2(dot(cross(Bv, A), G) / mpmath.sqrt(dot(G, G)), dot(A, Bv)))


def exact_term(case, pos, atoms, params, box=None, gvalues=None, budget=R.NO_ROUNDING, forces=True):
    """(E, bound of a double evaluation of the text, forces [arity][3]) of one term at 50 digits.  Raises expr_reference.Unstable
    where the text may jump within rounding."""
    kind = case['kind']
    main, defs = R.parse(case['text'])
    env = {k: float(v) for k, v in (case['globals'] if gvalues is None else gvalues).items()}
    env.update({name: float(p) for name, p in zip(case['names'], params)})
    atoms = [int(a) for a in atoms[:ARITY[kind]]]
    with mpmath.workdps(R.DIGITS):
        coords = [mpmath.mpf(float(pos[a][c])) for a in atoms for c in range(3)]

        def energy(cs, b=R.NO_ROUNDING):
            return R._evaluate_one(main, defs, dict(env, **_mp_variables(kind, cs, box)), b)
        value, bound = energy(coords, budget)
        f = np.zeros((len(atoms), 3))
        if forces:
            for q in range(len(coords)):
                f[q // 3, q % 3] = -float(mpmath.diff(lambda c: energy(coords[:q] + [c] + coords[q + 1:])[0], coords[q]))
    return value, bound, f


def term_sum(case, idx, params, positions, box=None, gvalues=None):
    """(energy, forces [n][3], per-term energies) of the reference over the terms `idx` (rows of atoms) with parameter rows `params`."""
    n = len(positions)
    forces = np.zeros((n, 3))
    energies = []
    with mpmath.workdps(R.DIGITS):
        for atoms, p in zip(idx, params):
            value, _, f = exact_term(case, positions, atoms, p, box, gvalues)
            energies.append(value)
            for role, a in enumerate(atoms[:ARITY[case['kind']]]):
                forces[int(a)] += f[role]
        total = float(mpmath.fsum(energies))
    return total, forces, np.array([float(e) for e in energies])


# ------------------------------------------------------------------------------------------------ the interpreter's leaves, restated
def run_term_program(prog, variables, params, gvalues, seed=0):
    """(E, dE/d variables[seed]) of a compile_term program in plain Python.  csrc/term_expr_vm.h gives the interpreter of
    pair_expr_vm.h other leaves: TERM_VAR k pushes (variables[k], 1 if k == seed else 0), TERM_P k pushes (params[k], 0).  That is
    the pair interpreter (pair_expr_cases.run_program) with r = the seeded variable, the other variables in the neighbour's slots and
    the parameters in the row atom's, which is how the words are rewritten here."""
    code = []
    for word in prog.code:
        op, arg = word & 0xff, word >> 8
        if op == X.ALL_OPCODES['TERM_VAR']:
            word = X.ALL_OPCODES['PAIR_R'] if arg == seed else X.ALL_OPCODES['PAIR_P2'] | arg << 8
        elif op == X.ALL_OPCODES['TERM_P']:
            word = X.ALL_OPCODES['PAIR_P1'] | arg << 8
        elif op in X.PAIR_OPCODES.values():
            raise ValueError('not a term-expression op: %d' % op)
        code.append(word)
    pair = X.Program()
    pair.code, pair.consts, pair.globals_ = code, prog.consts, prog.globals_
    return P.run_program(pair, float(variables[seed]), list(params), list(variables), gvalues)


# ------------------------------------------------------------------------------------------------ the terms of the GPU comparison
# texts no hand-written kind covers, each over terms of the emim-BCN4 fixture (2800 atoms; the System holds all of them)
GPU_CASES = ('morse', 'cosine-angle', 'rb-torsion', 'charmm-improper', 'position-restraint', 'flat-bottom')
GPU_TERMS = 48          # per text: 50-digit differentiation of every Cartesian component takes a tenth of a second per term
SEED = 20241019


def reference_terms(name, data):
    """(index rows [m][arity], parameter rows [m][n_params]) of the GPU comparison of text `name` on a fixture: the first GPU_TERMS
    usable terms of every 37th bond / angle / torsion (or every 37th atom) in file order, with parameters drawn from a fixed seed --
    from the fixture's own r0, theta0 and positions where the text has such a parameter, so that the energies are of ordinary size."""
    case = TEXTS[name]
    kind = case['kind']
    rng = np.random.default_rng(SEED + sum(map(ord, name)))
    pos, box = data['positions'], data['box']
    rows = {BOND: data['bonds'], ANGLE: data['angles'], TORSION: data['torsions'], EXTERNAL: np.arange(len(pos)).reshape(-1, 1)}[kind]
    idx, params = [], []
    for t in list(range(0, len(rows), 37)) + list(range(1, len(rows), 37)):
        atoms = [int(a) for a in rows[t]]
        if name == 'morse':
            p = [rng.uniform(200.0, 500.0), rng.uniform(15.0, 25.0), float(data['bond_r0'][t])]
        elif name == 'cosine-angle':
            p = [float(data['angle_theta0'][t]), rng.uniform(200.0, 800.0)]
        elif name == 'rb-torsion':
            p = list(rng.uniform(-10.0, 10.0, 6))
        elif name == 'charmm-improper':
            p = [rng.uniform(10.0, 200.0), rng.uniform(-3.0, 3.0)]
        elif name == 'position-restraint':
            p = [1000.0] + list(pos[atoms[0]] + rng.uniform(-0.05, 0.05, 3))
        else:           # flat-bottom: inside the well, outside it and -- the first term -- exactly at the anchor
            p = [rng.uniform(100.0, 1000.0), 0.1] + list(pos[atoms[0]] + (0.0 if not idx else 1.0) * rng.uniform(-0.2, 0.2, 3))
        if usable(case, pos, atoms, p, box if kind != EXTERNAL else None):
            idx.append(atoms)
            params.append([float(v) for v in p])
        if len(idx) == GPU_TERMS:
            break
    return np.array(idx, dtype=np.int32), np.array(params, dtype=np.float64)
