"""TEST INFRASTRUCTURE (checker only) of the compound-bond forces (csrc/compound.hip): texts of CustomCompoundBondForce /
CustomCentroidBondForce, and a reference at 50 digits.

Reference: per bond, every slot's position -- an atom, or the centre sum w_i x_i / sum w_i of a group of atoms over the raw
coordinates -- and from them the variables the text names (raw coordinates x1 .. zN, distance, the angle in [0, pi], the dihedral in
(-pi, pi] with PeriodicTorsionForce's sign; displacements take the minimum image when a box is given) are computed in mpmath at 50
digits; the calls of the TEXT are replaced by fresh names with a regular expression and the text is evaluated by
tests/expr_reference.py; every force component is -mpmath.diff of that energy in the Cartesian coordinate of the ATOM itself.  The
reference therefore shares neither the compiler, the interpreter, the analytic gradients nor the spread over a group's members.
(A variable no slot of which holds the displaced atom keeps its value: that saves time, not digits.)

Inputs to avoid (`usable`): angles within 1e-3 of 0 or pi, dihedrals with a (nearly) collinear triple or within 1e-3 of the cut of
atan2, and the kinks a text declares.  A test that filters asserts that it kept at least 95 % of its terms (`MIN_KEPT`).
"""
import math
import re

import mpmath
import numpy as np

import expr_reference as R

KINK_MARGIN = 1e-3
MIN_KEPT = 0.95
_CALL = re.compile(r'\b(distance|angle|dihedral)\s*\(\s*([pg]\d+)\s*,\s*([pg]\d+)\s*(?:,\s*([pg]\d+)\s*)?(?:,\s*([pg]\d+)\s*)?\)')
_COORD = re.compile(r"\b([xyz])([1-9]\d*)\b")
_V16 = ('kb*((distance(p1,p2)-r0)^2+(distance(p2,p3)-r0)^2+(distance(p3,p4)-r0)^2+(distance(p5,p6)-r0)^2+(distance(p7,p8)-r0)^2'
        '+0.01*(distance(p1,p8)-r0)^2)'
        ' + ka*((angle(p1,p2,p3)-t0)^2+(angle(p2,p3,p4)-t0)^2+(angle(p5,p6,p7)-t0)^2+(angle(p6,p7,p8)-t0)^2)'
        ' + kd*(cos(dihedral(p1,p2,p3,p4)-phi)+cos(2*dihedral(p5,p6,p7,p8)))'
        ' + kx*((x8-x1-dx)^2+(y8-y0)^2+(z8-z0)^2)')

# name -> slots per bond, text, per-bond parameter names, globals, kinks(values of the variables by name, parameters, globals)
TEXTS = {
    'harmonic-bond': dict(n=2, text='0.5*k*(distance(p1,p2)-r0)^2', names=['r0', 'k'], globals={}, kinks=lambda v, p, g: []),
    'harmonic-angle': dict(n=3, text='0.5*k*(angle(p1,p2,p3)-t0)^2', names=['t0', 'k'], globals={}, kinks=lambda v, p, g: []),
    'periodic-torsion': dict(n=4, text='k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0))', names=['n', 't0', 'k'], globals={}, kinks=lambda v, p, g: []),
    'urey-bradley': dict(n=3, text='0.5*k*(angle(p1,p2,p3)-t0)^2 + 0.5*kub*(distance(p1,p3)-d0)^2', names=['t0', 'k', 'd0', 'kub'], globals={},
                         kinks=lambda v, p, g: []),                                                                    # V = 2
    'torsion-14': dict(n=4, text='k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0)) + 0.5*kub*(distance(p1,p4)-d0)^2', names=['n', 't0', 'k', 'd0', 'kub'],
                       globals={}, kinks=lambda v, p, g: []),                                                          # V = 2
    'stretch-bend': dict(n=3, text='kss*(angle(p1,p2,p3)-t0)*((distance(p1,p2)-r1)+(distance(p3,p2)-r2)); kss = scale*k',
                         names=['k', 't0', 'r1', 'r2'], globals=dict(scale=1.25), kinks=lambda v, p, g: []),          # V = 3
    'five': dict(n=5, text='scale*(k1*(distance(p1,p2)-r0)^2 + k2*cos(dihedral(p1,p2,p3,p4)) + k3*(angle(p3,p4,p5)-t0)^2 + kz*abs(z5-z1))',
                 names=['k1', 'r0', 'k2', 'k3', 't0', 'kz'], globals=dict(scale=1.3),
                 kinks=lambda v, p, g: [v['z5'] - v['z1']]),                                                           # V = 5
    'sixteen': dict(n=8, text=_V16, names=['kb', 'r0', 'ka', 't0', 'kd', 'phi', 'kx', 'dx'], globals=dict(y0=1.0, z0=2.0),
                    kinks=lambda v, p, g: []),                                                                         # V = 16
    'centre-distance': dict(n=2, text='0.5*k*(distance(g1,g2)-d0)^2', names=['k', 'd0'], globals={}, kinks=lambda v, p, g: []),
    'centre-angle': dict(n=3, text='k*(1-cos(angle(g1,g2,g3)-t0)) + kx*(x1-x3)^2', names=['k', 't0'], globals=dict(kx=2.5),
                         kinks=lambda v, p, g: []),
}
N_VARIABLES = {'torsion-14': 2, 'harmonic-bond': 1, 'harmonic-angle': 1, 'periodic-torsion': 1, 'urey-bradley': 2, 'stretch-bend': 3, 'five': 5, 'sixteen': 16,
               'centre-distance': 1, 'centre-angle': 3}


def variables_in(text):
    """(rewritten text, {fresh name: (kind, slots)}) -- every call and every coordinate of the text, slots 0-based."""
    found = {}

    def call(m):
        slots = tuple(int(a[1:]) - 1 for a in m.groups()[1:] if a is not None)
        if len(slots) != dict(distance=2, angle=3, dihedral=4)[m.group(1)]:
            raise ValueError('wrong number of arguments: ' + m.group(0))
        name = '%s_%s' % (m.group(1), '_'.join(str(s + 1) for s in slots))
        found[name] = (m.group(1), slots)
        return name
    text = _CALL.sub(call, text)
    main = text.split(';')
    defined = {d.split('=')[0].strip() for d in main[1:]}
    for m in _COORD.finditer(text):
        if m.group(0) not in defined:
            found[m.group(0)] = (m.group(1), (int(m.group(2)) - 1,))
    return text, found


# ------------------------------------------------------------------------------------------------ geometry: one code, any arithmetic
def _variable(kind, x, box, sqrt, acos, atan2, nint, number):
    """The variable of `kind` over the slot positions x (lists of three numbers of one arithmetic)."""
    def delta(a, b):
        d = [p - q for p, q in zip(x[a], x[b])]
        if box is not None:
            d = [c - number(float(L)) * nint(c / number(float(L))) for c, L in zip(d, box)]
        return d

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    if kind in 'xyz':
        return x[0]['xyz'.index(kind)]
    if kind == 'distance':
        d = delta(0, 1)
        return sqrt(dot(d, d))
    if kind == 'angle':
        d1, d2 = delta(0, 1), delta(2, 1)
        return acos(dot(d1, d2) / sqrt(dot(d1, d1) * dot(d2, d2)))
    F, G, H = delta(0, 1), delta(1, 2), delta(3, 2)
    A, Bv = cross(F, G), cross(H, G)
    return atan2(dot(cross(Bv, A), G) / sqrt(dot(G, G)), dot(A, Bv))


def _float_variable(kind, x, box):
    return float(_variable(kind, x, box, math.sqrt, lambda c: math.acos(max(-1.0, min(1.0, c))), math.atan2, round, float))


def centre(pos, atoms, weights):
    """Weighted centre in fp64 (selection and closed forms only)."""
    w = np.asarray(weights, dtype=np.float64)
    return (w[:, None] * np.asarray(pos, dtype=np.float64)[list(atoms)]).sum(axis=0) / w.sum()


def slot_positions(pos, members):
    """fp64 positions of a bond's slots: members[s] is an atom index, or (atoms, weights) of a group."""
    return [list(centre(pos, *m)) if isinstance(m, tuple) else [float(c) for c in pos[int(m)]] for m in members]


def float_variables(case, pos, members, box=None):
    """{name: value} of the text's variables in fp64 (for choosing inputs, never as the reference of a comparison)."""
    x = slot_positions(pos, members)
    return {name: _float_variable(kind, [x[s] for s in slots], box) for name, (kind, slots) in variables_in(case['text'])[1].items()}


def usable(case, pos, members, params, box=None, gvalues=None):
    """True when the bond is none of the inputs to avoid."""
    x = slot_positions(pos, members)
    values = {}
    for name, (kind, slots) in variables_in(case['text'])[1].items():
        v = values[name] = _float_variable(kind, [x[s] for s in slots], box)
        if kind == 'angle' and not (KINK_MARGIN < v < math.pi - KINK_MARGIN):
            return False
        if kind == 'dihedral':
            y = [np.array(x[s]) for s in slots]
            for i, j, k in ((0, 1, 2), (1, 2, 3)):
                d1, d2 = y[i] - y[j], y[k] - y[j]
                if box is not None:
                    d1, d2 = d1 - np.asarray(box) * np.rint(d1 / np.asarray(box)), d2 - np.asarray(box) * np.rint(d2 / np.asarray(box))
                if np.linalg.norm(np.cross(d1, d2)) / math.sqrt(d1.dot(d1) * d2.dot(d2)) < 0.05:
                    return False
            if abs(abs(v) - math.pi) < KINK_MARGIN:          # the cut of atan2
                return False
    g = dict(case['globals'] if gvalues is None else gvalues)
    return all(abs(q) > KINK_MARGIN for q in case['kinks'](values, list(params), g))


# ------------------------------------------------------------------------------------------------ the reference, mpmath
def _mp_variable(kind, x, box):
    return _variable(kind, x, box, mpmath.sqrt, mpmath.acos, mpmath.atan2, mpmath.nint, mpmath.mpf)


def exact_bond(case, pos, members, params, box=None, gvalues=None, forces=True):
    """(E, {atom: force[3]}, {name: variable at 50 digits}) of one bond.  members[s]: an atom index, or (atoms, weights) of a group."""
    text, table = variables_in(case['text'])
    main, defs = R.parse(text)
    env = {k: float(v) for k, v in (case['globals'] if gvalues is None else gvalues).items()}
    env.update({name: float(p) for name, p in zip(case['names'], params)})
    groups = [(([int(a) for a in m[0]], [float(w) for w in m[1]]) if isinstance(m, tuple) else ([int(m)], [1.0])) for m in members]
    atoms = sorted({a for g in groups for a in g[0]})
    with mpmath.workdps(R.DIGITS):
        coords = {a: [mpmath.mpf(float(c)) for c in pos[a]] for a in atoms}

        def slot(s, moved=None):
            members_, weights = groups[s]
            W = mpmath.fsum(mpmath.mpf(w) for w in weights)
            out = []
            for c in range(3):
                terms = []
                for a, w in zip(members_, weights):
                    value = moved[2] if moved is not None and moved[0] == a and moved[1] == c else coords[a][c]
                    terms.append(mpmath.mpf(w) * value)
                out.append(mpmath.fsum(terms) / W)
            return out
        base_slots = [slot(s) for s in range(len(groups))]
        base = {name: _mp_variable(kind, [base_slots[s] for s in slots], box) for name, (kind, slots) in table.items()}
        value = R._evaluate_one(main, defs, dict(env, **base), R.NO_ROUNDING)[0]
        out = {}
        if forces:
            for a in atoms:
                touched = [s for s, g in enumerate(groups) if a in g[0]]
                f = []
                for c in range(3):
                    def energy(t, a=a, c=c):
                        x = list(base_slots)
                        for s in touched:
                            x[s] = slot(s, (a, c, t))
                        values = dict(base)
                        for name, (kind, slots) in table.items():
                            if set(slots) & set(touched):
                                values[name] = _mp_variable(kind, [x[s] for s in slots], box)
                        return R._evaluate_one(main, defs, dict(env, **values), R.NO_ROUNDING)[0]
                    f.append(-float(mpmath.diff(energy, coords[a][c])))
                out[a] = np.array(f)
        return value, out, base


def bond_sum(case, rows, params, positions, box=None, gvalues=None):
    """Per-bond (energies as mpf, forces [n_bonds] of {atom: force}) of the reference over the bonds `rows` (lists of members)."""
    energies, forces = [], []
    for members, p in zip(rows, params):
        e, f, _ = exact_bond(case, positions, members, p, box, gvalues)
        energies.append(e)
        forces.append(f)
    return energies, forces


def total(energies, forces, n, count=None):
    """(energy, forces [n][3]) of the first `count` bonds of bond_sum's answer."""
    count = len(energies) if count is None else count
    out = np.zeros((n, 3))
    for f in forces[:count]:
        for a, v in f.items():
            out[a] += v
    with mpmath.workdps(R.DIGITS):
        return float(mpmath.fsum(energies[:count])), out


# ------------------------------------------------------------------------------------------------ the bonds of the comparisons
SEED = 20241020


def fixture_rows(name, data, count):
    """(rows, parameter rows, candidates looked at) of text `name` over a fixture: bonds made from the fixture's own angle and torsion
    lists in file order with a stride -- 2 and 3 particles from an angle, 4 from a torsion, 5 and 8 from a torsion plus the first atom /
    all of the torsion 1000 rows further on (another molecule) --, parameters drawn from a fixed seed around the fixture's own geometry."""
    case = TEXTS[name]
    rng = np.random.default_rng(SEED + sum(map(ord, name)))
    pos, box = data['positions'], data['box']
    angles, torsions = data['angles'], data['torsions']
    rows, params, looked = [], [], 0
    t = 0
    while len(rows) < count:
        if case['n'] <= 3:
            members = [int(a) for a in angles[(37 * t) % len(angles)][:case['n']]] if case['n'] == 3 else [int(a) for a in angles[(37 * t) % len(angles)][:2]]
        else:
            first, second = torsions[(41 * t) % len(torsions)], torsions[(41 * t + 1000) % len(torsions)]
            members = [int(a) for a in first] + [int(a) for a in second][:case['n'] - 4]
        t += 1
        if len(set(members)) != len(members):
            continue
        looked += 1
        v = float_variables(case, pos, members, box)
        pick = dict(
            r0=lambda: v.get('distance_1_2', 0.15) + rng.uniform(-0.01, 0.01), r1=lambda: v.get('distance_1_2', 0.15) + rng.uniform(-0.01, 0.01),
            r2=lambda: v.get('distance_3_2', 0.15) + rng.uniform(-0.01, 0.01), d0=lambda: v.get('distance_1_3', v.get('distance_1_4', 0.2)) + rng.uniform(-0.01, 0.01),
            t0=lambda: rng.uniform(1.7, 2.1), phi=lambda: rng.uniform(-3.0, 3.0), n=lambda: float(rng.integers(1, 5)),
            dx=lambda: rng.uniform(-0.2, 0.2))
        p = [pick[q]() if q in pick else rng.uniform(50.0, 500.0) for q in case['names']]
        if usable(case, pos, members, p, box):
            rows.append(members)
            params.append([float(q) for q in p])
    return rows, np.array(params, dtype=np.float64), looked
