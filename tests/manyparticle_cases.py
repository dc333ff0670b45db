"""TEST INFRASTRUCTURE (checker only) of the many-particle force (csrc/manyparticle.hip): texts of CustomManyParticleForce over sets of
three, the sets that count on the host, the permutation the type filters choose, and the way to the 50-digit reference of
tests/compound_cases.py.

The rules are the project's.  A set is three distinct particles no pair of which is excluded.  SinglePermutation:
every unordered set once, and with a cutoff all three distances below it; its tuple is the particles in ascending order.
UniqueCentralParticle: every set once per centre c, and with a cutoff the two distances from c below it (the satellites' distance is
not tested); its tuple is the centre, then the satellites ascending.  The permutations of the tuple are taken in lexicographic order
(central mode keeps the centre at p1); the first whose particles satisfy every role's type filter is evaluated, and a set with none
is skipped.  All of it is enumerated here in fp64, with loops over particles and itertools.permutations: it shares neither the
neighbour table, the queue nor the table over dense type indices of the engine.

A set that counts is one bond of three particles of tests/compound_cases.py -- the text already reads p1 p2 p3 and x1 .. z3 -- with
the per-particle parameters of p1, p2, p3 concatenated under the names <name>1 <name>2 <name>3; compound_cases.exact_bond (the text at
50 digits, forces by mpmath.diff in the atoms' own coordinates) is the reference.

Inputs to avoid (`usable`): a tested pair within 1e-6 nm of the cutoff, and what compound_cases.usable avoids.  A test that filters
asserts that it kept at least 95 % of its sets (`MIN_KEPT`); the seeds below are chosen so that the reference alone meets that, and
tests/test_manyparticle_host.py checks it on the CPU.
"""
import itertools

import numpy as np

import compound_cases as C

MIN_KEPT = C.MIN_KEPT
CUTOFF_MARGIN = 1e-6

_V16 = ('kb*((distance(p1,p2)-r0)^2+0.5*(distance(p1,p3)-r0)^2+0.3*(distance(p2,p3)-r0)^2+0.1*(distance(p2,p1)-0.2)^2+0.05*distance(p3,p1))'
        ' + ka*((angle(p1,p2,p3)-t0)^2+0.5*(angle(p2,p1,p3)-t0)^2+0.2*(angle(p1,p3,p2)-t0)^2+0.1*cos(angle(p3,p2,p1)))'
        ' + kt*cos(dihedral(p1,p2,p3,p1)-phi)'
        ' + kx*((x1-x3)^2+(y2-y1)^2+0.5*(z3-z1)^2)')

# name -> text, per-particle parameter names, globals.  'distance', 'three', 'sixteen' and 'parameters' are NOT symmetric in the
# particles: their sums depend on the permutation the rule chooses.
TEXTS = {
    'axilrod-teller': dict(text='C*(1+3*cos(angle(p1,p2,p3))*cos(angle(p2,p3,p1))*cos(angle(p3,p1,p2)))/(distance(p1,p2)*distance(p2,p3)*distance(p1,p3))^3',
                           names=[], globals=dict(C=0.02)),                                                                     # V = 6
    # the three-body term of Stillinger-Weber with the angle at p1 (the mW water model's numbers; the cutoff is a*sig = 0.43065 nm)
    'stillinger-weber': dict(text='eps*lam*(cos(angle(p2,p1,p3))+1/3)^2*exp(gam*sig/(distance(p1,p2)-a*sig)+gam*sig/(distance(p1,p3)-a*sig))',
                             names=[], globals=dict(eps=25.895, lam=23.15, gam=1.2, sig=0.23925, a=1.8)),                       # V = 3
    'distance': dict(text='k*(distance(p1,p2)-r0)^2', names=[], globals=dict(k=40.0, r0=0.3)),                                 # V = 1
    'three': dict(text='k*(distance(p1,p2)-r0)^2*(1.5+cos(angle(p2,p1,p3)))*(1+distance(p1,p3))', names=[], globals=dict(k=25.0, r0=0.3)),   # V = 3
    'with-dihedral': dict(text='k*(distance(p1,p2)-r0)^2*(2+cos(dihedral(p1,p2,p3,p1)-phi))*(1+cos(angle(p1,p2,p3)))', names=[],
                          globals=dict(k=25.0, r0=0.3, phi=0.7)),                                                              # V = 3
    'sixteen': dict(text=_V16, names=[], globals=dict(kb=30.0, r0=0.35, ka=4.0, t0=1.9, kt=3.0, phi=0.4, kx=2.0)),              # V = 16
    'parameters': dict(text='scale*eps1*eps2*eps3*(distance(p1,p2)-sig1-0.5*sig2)^2*(1.5+cos(angle(p2,p1,p3)-sig3))', names=['sig', 'eps'],
                       globals=dict(scale=1.2)),                                                                                # V = 2
}
N_VARIABLES = {'axilrod-teller': 6, 'stillinger-weber': 3, 'distance': 1, 'three': 3, 'with-dihedral': 3, 'sixteen': 16, 'parameters': 2}
PARAMETER_RANGE = dict(sig=(0.1, 0.2), eps=(1.0, 3.0))
SW_CUTOFF = 1.8 * 0.23925
PERMUTATIONS = list(itertools.permutations(range(3)))          # lexicographic


def compound_case(name, gvalues=None):
    """The case of tests/compound_cases.py that restates text `name`: three particles, the parameters of p1, p2, p3 concatenated."""
    case = TEXTS[name]
    return dict(n=3, text=case['text'], names=['%s%d' % (p, r + 1) for r in range(3) for p in case['names']],
                globals=dict(case['globals'] if gvalues is None else gvalues), kinks=lambda v, p, g: [])


def parameters(name, n, seed):
    """[n][parameters] of the particles of text `name`, drawn from a fixed seed."""
    names = TEXTS[name]['names']
    rng = np.random.default_rng(seed)
    return np.array([[rng.uniform(*PARAMETER_RANGE[p]) for p in names] for _ in range(n)], dtype=np.float64).reshape(n, len(names))


def set_parameters(par, members):
    return [float(v) for m in members for v in par[m]]


def positions(n, edge, seed, min_distance=0.15, place=None):
    """[n][3]: uniformly in a cube of `edge`, or where place(rng, t) puts particle t; no two closer than min_distance under the
    minimum image of `edge`."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3))
    for t in range(n):
        while True:
            x = rng.uniform(0.0, edge, 3) if place is None else np.asarray(place(rng, t), dtype=np.float64)
            if t:
                d = pos[:t] - x
                d -= edge * np.rint(d / edge)
                if np.sqrt((d ** 2).sum(axis=1)).min() < min_distance:
                    continue
            break
        pos[t] = x
    return pos


def ball(rng, centre, radius):
    v = rng.normal(size=3)
    return np.asarray(centre) + v / np.linalg.norm(v) * radius * rng.uniform() ** (1.0 / 3.0)


def distances(pos, box=None):
    """|x_i - x_j| of every pair in fp64, [n][n]; the minimum image when a box is given."""
    d = np.asarray(pos)[:, None, :] - np.asarray(pos)[None, :, :]
    if box is not None:
        d = d - np.asarray(box) * np.rint(d / np.asarray(box))
    return np.sqrt((d ** 2).sum(axis=2))


def margin_ok(pos, cutoff, box=None):
    """No pair of the layout within CUTOFF_MARGIN of the cutoff (the host's and the kernel's lists then agree)."""
    return not (np.abs(distances(pos, box) - cutoff) < CUTOFF_MARGIN).any()


def first_permutation(tuple_types, filters, central):
    """The first permutation of the tuple, in lexicographic order, whose types satisfy every role's filter (an empty filter takes
    any type); None when there is none.  Central mode keeps the centre at p1."""
    for perm in PERMUTATIONS:
        if central and perm[0] != 0:
            continue
        if all(not filters[r] or tuple_types[perm[r]] in filters[r] for r in range(3)):
            return perm
    return None


def permutation_table(filters, types, central):
    """[T][T][T] over the dense indices of the sorted distinct `types`: the position of first_permutation in PERMUTATIONS, or -1."""
    T = len(types)
    table = np.full((T, T, T), -1, dtype=np.int32)
    for a, b, c in itertools.product(range(T), repeat=3):
        perm = first_permutation((types[a], types[b], types[c]), filters, central)
        if perm is not None:
            table[a, b, c] = PERMUTATIONS.index(perm)
    return table


def neighbours(pos, exclusions=(), cutoff=None, box=None):
    """[n] sorted lists: the particles j != i that are not excluded from i and, with a cutoff, inside it."""
    n = len(pos)
    r = distances(pos, box)
    ex = {frozenset(e) for e in exclusions}
    return [[j for j in range(n) if j != i and frozenset((i, j)) not in ex and (cutoff is None or r[i, j] < cutoff)] for i in range(n)]


def enumerate_sets(pos, central, exclusions=(), cutoff=None, box=None, types=None, filters=None):
    """The evaluations of the text as (p1, p2, p3), in the order of the rule: SinglePermutation i < j < k, UniqueCentralParticle
    centre by centre and j < k."""
    n = len(pos)
    r = distances(pos, box)
    ex = {frozenset(e) for e in exclusions}
    types = [0] * n if types is None else list(types)
    filters = [set(), set(), set()] if filters is None else [set(f) for f in filters]

    def inside(a, b):
        return cutoff is None or r[a, b] < cutoff

    def allowed(a, b):
        return frozenset((a, b)) not in ex
    out = []
    if central:
        for c in range(n):
            for j in range(n):
                for k in range(j + 1, n):
                    if c in (j, k) or not (allowed(c, j) and allowed(c, k) and allowed(j, k) and inside(c, j) and inside(c, k)):
                        continue
                    members = (c, j, k)
                    perm = first_permutation([types[m] for m in members], filters, True)
                    if perm is not None:
                        out.append(tuple(members[p] for p in perm))
    else:
        for i in range(n):
            for j in range(i + 1, n):
                if not (allowed(i, j) and inside(i, j)):
                    continue
                for k in range(j + 1, n):
                    if not (allowed(i, k) and allowed(j, k) and inside(i, k) and inside(j, k)):
                        continue
                    members = (i, j, k)
                    perm = first_permutation([types[m] for m in members], filters, False)
                    if perm is not None:
                        out.append(tuple(members[p] for p in perm))
    return out


def entries_per_owner(sets, n):
    """How many evaluations contain each particle: what the particle's wavefront queues."""
    count = np.zeros(n, dtype=np.int64)
    for members in sets:
        for m in members:
            count[m] += 1
    return count


def usable(name, pos, members, params, cutoff=None, box=None, central=False):
    """True when the set is none of the inputs to avoid.  members: (p1, p2, p3); in central mode p1 is the centre."""
    if cutoff is not None:
        r = distances(np.asarray(pos)[list(members)], box)
        tested = ((0, 1), (0, 2)) if central else ((0, 1), (0, 2), (1, 2))
        if any(abs(r[a, b] - cutoff) < CUTOFF_MARGIN for a, b in tested):
            return False
    return C.usable(compound_case(name), pos, list(members), params, box)


def reference(name, pos, sets, par, cutoff=None, box=None, central=False, gvalues=None, cache=None):
    """(energy, forces [n][3], sets kept, sets looked at) of the 50-digit reference over the usable sets of `sets`.  cache: a dict
    that keeps the bonds already computed (the same set under another method is the same bond while the box is the same)."""
    case = compound_case(name, gvalues)
    kept, energies, forces = [], [], []
    for members in sets:
        p = set_parameters(par, members)
        if not usable(name, pos, members, p, cutoff, box, central):
            continue
        key = (name, tuple(members), None if box is None else tuple(float(b) for b in box))
        if cache is None or key not in cache:
            e, f, _ = C.exact_bond(case, pos, list(members), p, box, gvalues)
            if cache is not None:
                cache[key] = (e, f)
        else:
            e, f = cache[key]
        kept.append(tuple(members))
        energies.append(e)
        forces.append(f)
    e, f = C.total(energies, forces, len(pos))
    return e, f, kept, len(sets)


# ------------------------------------------------------------------------------------------------ the layouts of the comparisons
SMALL_EDGE, SMALL_CUTOFF = 2.0, 0.7
SMALL_SEEDS = {3: 1, 4: 1, 6: 1}             # tests/test_manyparticle_host.py: the filter keeps 95 % with these


def small_layout(n, periodic):
    """n = 3, 4, 6 particles in a ball of 0.45 nm -- in the middle of the 2 nm box, or for the periodic method around its corner: most
    pairs then lie inside the 0.7 nm cutoff only by the minimum image."""
    centre = np.zeros(3) if periodic else np.full(3, 0.5 * SMALL_EDGE)
    return positions(n, SMALL_EDGE, SMALL_SEEDS[n], 0.2, lambda rng, t: ball(rng, centre, 0.45) % SMALL_EDGE)


def cluster_layout(m, rc, seed, extra=0):
    """Particle 0 and m more in a ball of 0.45 rc around it (all within the cutoff of one another), then `extra` particles far away."""
    def place(rng, t):
        if t <= m:
            return np.array([1.0, 1.0, 1.0]) + (ball(rng, (0.0, 0.0, 0.0), 0.45 * rc) if t else 0.0)
        return np.array([1.0, 1.0, 1.0]) + 3.0 * rc * (t - m + 1) * np.array([1.0, 0.3, 0.2])
    return positions(m + 1 + extra, 1e9, seed, min(0.1, 0.25 * rc), place)


def rows_layout(rc):
    """18 particles under a cutoff: a pair (neighbour rows of length 1: no set), a triple (rows of length 2: one pair of
    neighbours) and a cluster of 13 (rows of length 12: 66 pairs, more than one batch), far from one another."""
    def place(rng, t):
        group = 0 if t < 2 else (1 if t < 5 else 2)
        return np.array([1.0 + 4.0 * rc * group, 1.0, 1.0]) + ball(rng, (0.0, 0.0, 0.0), 0.45 * rc)
    return positions(18, 1e9, 17, min(0.1, 0.2 * rc), place)
