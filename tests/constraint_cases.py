"""tests/constraint_cases.py -- constraint sets for the tests of the SHAKE / RATTLE sweeps (csrc/cons_sweeps.h): rigid clusters with
cycles, clusters at the 8-atom / 16-constraint limits, scalene triangles in every listing, unfriendly atom numberings, and inputs
on which the solvers must fail.  Plain numpy, seeded, no GPU.  TEST INFRASTRUCTURE ONLY.

A case is a dict: x0 [n][3] (on the constraint surface), mass [n], pairs [nc][2] (global indices, int32), dist [nc] (every one
computed from x0, so that a set is consistent by construction), clusters (per cluster: its shape's name, its atoms in the builder's
order, its constraints as pairs of positions in that list in listing order, their distances) and free (the atoms of no cluster).
Every cluster has a random rotation and a random place in a 6 nm box."""
import functools
import itertools

import numpy as np

import stock_ref as SR

SIGMA = 0.003            # nm: the perturbation of the existing solver tests
BOX = 6.0
KT = 0.00831446261815324 * 300.0
DT, SEED, STEPS = 0.002, 20261, 3
FRICTION = {SR.VERLET: 0.0, SR.LANGEVIN_MIDDLE: 5.0, SR.LANGEVIN: 5.0, SR.BROWNIAN: 100.0}       # 1/ps, as test_gpu_stock.py
CAP = 350                # sweeps the restatement may use on any committed input: well inside the solvers' 500

R_OH, R_HH, R_XH, R_CC = 0.09572, 0.15139, 0.109, 0.153
TETRAHEDRON = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
ALL_PAIRS = lambda n: list(itertools.combinations(range(n), 2))      # noqa: E731
WATER_ORDERS = [[(1, 0), (2, 0), (1, 2)], [(0, 1), (0, 2), (1, 2)], [(1, 2), (0, 1), (2, 0)]]      # (those of test_gpu_stock.py)
SCALENE_VARIANTS = [(order, flips) for order in itertools.permutations(range(3)) for flips in range(8)]
RIGID = ['methyl', 'methane', 'ring6', 'ring8', 'scalene']          # the shapes this file adds
KNOWN = ['water', 'pair', 'xh3', 'chain8']                          # the shapes the suite had


def _unit_vector(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def _ring(n_atoms):
    k = np.arange(n_atoms)
    xs = np.stack([0.14 * np.cos(2 * np.pi * k / n_atoms), 0.14 * np.sin(2 * np.pi * k / n_atoms), 0.02 * (-1.0) ** k], axis=1)
    local = [(i, (i + 1) % n_atoms) for i in range(n_atoms)] + [(i, (i + 2) % n_atoms) for i in range(n_atoms)]
    return xs, [12.011 + 1.5 * (i % 3) for i in range(n_atoms)], local


def shape(name, variant, rng):
    """One cluster in its own frame: (positions, masses, local pairs in listing order).  variant: which listing of the shapes
    that have several (scalene: 0 .. 47; water: 0 .. 2; pair: 0 .. 1)."""
    if name == 'methyl':         # C + 3 H of a tetrahedral centre: 3 C-H + 3 H-H
        return np.vstack([np.zeros(3), R_XH * TETRAHEDRON[:3]]), [12.011, 1.008, 1.008, 1.008], ALL_PAIRS(4)
    if name == 'methane':        # 4 C-H + 6 H-H: one constraint more than the body has internal coordinates
        return np.vstack([np.zeros(3), R_XH * TETRAHEDRON]), [12.011] + [1.008] * 4, ALL_PAIRS(5)
    if name == 'ring6':          # puckered ring, bonds + 1-3 distances: 12 constraints on 6 atoms
        return _ring(6)
    if name == 'ring8':          # 16 constraints on 8 atoms: both limits of a cluster
        return _ring(8)
    if name == 'scalene':        # three different sides, three different masses, one of the 6 orders x 8 orientations
        order, flips = SCALENE_VARIANTS[variant % 48]
        base = [(0, 1), (0, 2), (1, 2)]
        local = [base[q][::-1] if flips >> k & 1 else base[q] for k, q in enumerate(order)]
        return np.array([[0.0, 0.0, 0.0], [0.11, 0.0, 0.0], [0.03, 0.14, 0.0]]), [14.0067, 1.008, 3.5], local
    if name == 'water':
        half = np.arcsin(0.5 * R_HH / R_OH)
        xs = np.array([[0.0, 0.0, 0.0], [R_OH * np.cos(half), R_OH * np.sin(half), 0.0], [R_OH * np.cos(half), -R_OH * np.sin(half), 0.0]])
        return xs, [15.9994, 1.008, 1.008], WATER_ORDERS[variant % 3]
    if name == 'pair':
        return np.array([[0.0, 0.0, 0.0], [R_XH, 0.0, 0.0]]), [12.011, 1.008], [(1, 0) if variant % 2 else (0, 1)]
    if name == 'xh3':            # a star with unequal masses and three random directions
        return (np.vstack([np.zeros(3)] + [R_XH * _unit_vector(rng) for _ in range(3)]), [14.0067, 1.008, 1.508, 2.008],
                [(0, 1), (0, 2), (0, 3)])
    if name == 'chain8':         # an open chain at the atom limit
        xs = [np.zeros(3)]
        for _ in range(7):
            xs.append(xs[-1] + R_CC * _unit_vector(rng))
        return np.array(xs), [12.011] + [12.011 + 1.5 * (k % 3) for k in range(7)], [(k, k + 1) for k in range(7)]
    raise ValueError(name)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def assemble(specs, seed):
    """specs: [(shape name, variant)] or 'free', in the order of the atoms.  Distances are those of x0."""
    rng = np.random.default_rng(seed)
    xs, ms, pairs, clusters, free = [], [], [], [], []
    for spec in specs:
        base, origin = len(xs), rng.uniform(0.0, BOX, 3)
        if spec == 'free':
            free.append(base)
            xs.append(origin)
            ms.append(float(rng.choice([1.008, 12.011, 15.9994, 35.453])))
            continue
        p, m, local = shape(spec[0], spec[1], rng)
        xs += list(origin + p @ _rotation(rng).T)
        ms += list(m)
        pairs += [(base + i, base + j) for i, j in local]
        clusters.append((spec[0], list(range(base, base + len(m))), [tuple(q) for q in local]))
    x0, mass, pairs = np.array(xs), np.array(ms), np.array(pairs, dtype=np.int32).reshape(-1, 2)
    dist = np.linalg.norm(x0[pairs[:, 0]] - x0[pairs[:, 1]], axis=1)
    return _finish(dict(x0=x0, mass=mass, pairs=pairs, dist=dist, free=free, clusters=clusters))


def _finish(case):
    """(the per-cluster distances, from the case's x0)"""
    x0 = case['x0']
    case['clusters'] = [(c[0], c[1], c[2], [float(np.linalg.norm(x0[c[1][i]] - x0[c[1][j]])) for i, j in c[2]]) for c in case['clusters']]
    case['free'] = np.array(case['free'], dtype=int)
    return case


def instances(name, count, seed):
    """count clusters of one shape (every listing in turn), molecule by molecule."""
    return assemble([(name, k) for k in range(count)], seed)


def shuffled(counts, seed):
    """counts: {shape or 'free': how many}; the molecules in random order."""
    specs = []
    for name, count in counts.items():
        specs += ['free'] * count if name == 'free' else [(name, k) for k in range(count)]
    order = np.random.default_rng(seed).permutation(len(specs))
    return assemble([specs[k] for k in order], seed + 1)


@functools.lru_cache(maxsize=None)
def mixed():
    """16 of each rigid shape (all 48 scalene listings), 30 waters, 17 free atoms: 619 atoms."""
    return shuffled({'methyl': 16, 'methane': 16, 'ring6': 16, 'ring8': 16, 'scalene': 48, 'water': 30, 'free': 17}, 4101)


@functools.lru_cache(maxsize=None)
def triangles():
    """The 48 scalene listings and 16 waters: 64 clusters that amm_constraints_create classes as triangles."""
    return shuffled({'scalene': 48, 'water': 16}, 4201)


def census(n_tri, n_two, n_gen, n_free, seed=4301):
    """A set with that many units of each class of k_stock; the generic clusters are X-H3 stars, methyls and 8-atom chains in turn."""
    specs = [('water' if k % 2 else 'scalene', k) for k in range(n_tri)] + [('pair', k) for k in range(n_two)]
    specs += [(['xh3', 'methyl', 'chain8'][k % 3], k) for k in range(n_gen)] + ['free'] * n_free
    order = np.random.default_rng(seed).permutation(len(specs))
    return assemble([specs[k] for k in order], seed + 1)


# ------------------------------------------------------------------------------------ layouts
def scatter(case, seed):
    """Renumber the atoms by a random permutation: atom a becomes perm[a].  A cluster's atoms end up spread through the index range;
    its constraints keep their order and their orientation.  Returns (case, perm)."""
    n = len(case['x0'])
    perm = np.random.default_rng(seed).permutation(n)
    x0, mass = np.empty_like(case['x0']), np.empty_like(case['mass'])
    x0[perm], mass[perm] = case['x0'], case['mass']
    out = dict(x0=x0, mass=mass, pairs=perm[case['pairs']].astype(np.int32), dist=case['dist'].copy(), free=perm[case['free']],
               clusters=[(name, [int(perm[a]) for a in atoms], local) for name, atoms, local, _ in case['clusters']])
    return _finish(out), perm


def interleave_constraints(case, seed):
    """Shuffle the global constraint list, keeping the relative order of each cluster's constraints."""
    owner = np.empty(len(case['pairs']), dtype=int)
    of_atom = {a: c for c, (_, atoms, _, _) in enumerate(case['clusters']) for a in atoms}
    for q, (i, _) in enumerate(case['pairs']):
        owner[q] = of_atom[int(i)]
    slots = np.random.default_rng(seed).permutation(owner)          # which cluster speaks at each place of the new list
    queues = {c: list(np.flatnonzero(owner == c)) for c in range(len(case['clusters']))}
    order = np.array([queues[c].pop(0) for c in slots], dtype=int)
    out = dict(case)
    out['pairs'], out['dist'] = case['pairs'][order], case['dist'][order]
    return out


@functools.lru_cache(maxsize=None)
def mixed_scattered():
    case, perm = scatter(mixed(), 4102)
    return interleave_constraints(case, 4103), perm


# ------------------------------------------------------------------------------------ inputs and restated results, computed once
def clusters_of(case, regroup=True):
    """stock_ref.Clusters of the case.  regroup: the batches that are swept together are formed by listing alone -- a cluster's atoms
    labelled in the order in which its constraints name them -- not by the atoms' rank in the numbering, so that a scattered set
    is swept in as few batches as the plain one.  The arithmetic per cluster is the same (test_constraint_cases_host.py)."""
    cl = SR.Clusters(len(case['x0']), case['pairs'], case['dist'])
    if regroup:
        batches = {}
        for idx, local, d in cl.list:
            label = {}
            for a in itertools.chain.from_iterable(local):
                label.setdefault(a, len(label))
            key = (len(idx), tuple((label[i], label[j]) for i, j in local))
            batches.setdefault(key, []).append(([idx[a] for a in sorted(label, key=label.get)], d))
        cl.batches = [(np.array([idx for idx, _ in members]), list(key[1]), np.array([d for _, d in members]))
                      for key, members in batches.items()]
    return cl


def moved(case, seed=1):
    return case['x0'] + np.random.default_rng(seed).normal(0.0, SIGMA, case['x0'].shape)


def velocities(case, seed=2):
    return np.random.default_rng(seed).normal(0.0, 0.5, case['x0'].shape)


def thermal(case, seed=3):
    """(v, f) for a stock step: Maxwell velocities at 300 K and a fixed random force buffer, as test_gpu_stock.py has them."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=case['x0'].shape) * np.sqrt(KT / case['mass'])[:, None], rng.normal(0.0, 300.0, case['x0'].shape)


def restated_solvers(case, tol, x=None, v=None):
    """SAVE_REF at x0 ; x = moved ; CONSTRAIN_X ; CONSTRAIN_V.  Returns (x', v', sweeps of SHAKE, sweeps of RATTLE)."""
    cl = clusters_of(case)
    xs, ns = SR.shake(moved(case) if x is None else x, case['x0'], case['mass'], cl, tol)
    vs, nr = SR.rattle(xs, velocities(case) if v is None else v, case['mass'], cl, tol)
    return xs, vs, ns, nr


def restated_steps(case, kind, tol, steps=STEPS, v=None, f=None):
    """The states after steps 1 .. steps of stock_ref.step from (x0, thermal velocities), and the most sweeps a solver call used."""
    cl = clusters_of(case) if len(case['pairs']) else None
    v0, f0 = thermal(case)
    x, v, f, worst, states = case['x0'], v0 if v is None else v, f0 if f is None else f, 0, []
    for k in range(1, steps + 1):
        x, v, sweeps = SR.step(kind, x, v, f, case['mass'], cl, DT, FRICTION[kind], KT, tol, SEED, k)
        worst = max(worst, sweeps)
        states.append((x, v))
    return states, worst


def oracle_distances(case, xin, xref, xs, vin, vs, skip=('methane',)):
    """Largest distance of (xs, vs) from the exact solutions of the constraint equations (oracle/constraints_oracle.py), per shape:
    {name: [nm, nm/ps]}.  xs = SHAKE of xin along xref; vs = RATTLE of vin at xs (None: positions only)."""
    from oracle import constraints_oracle as CO
    worst = {}
    for name, atoms, local, dist in case['clusters']:
        if name in skip:
            continue
        m = case['mass'][atoms]
        dx = np.abs(xs[atoms] - CO.shake_exact(xin[atoms], xref[atoms], m, local, dist)).max()
        dv = np.abs(vs[atoms] - CO.rattle_exact(xs[atoms], vin[atoms], m, local)).max() if vs is not None else 0.0
        w = worst.setdefault(name, [0.0, 0.0])
        w[0], w[1] = max(w[0], dx), max(w[1], dv)
    return worst


# ------------------------------------------------------------------------------------ inputs on which the solvers must fail
def with_waters(x_extra, m_extra, pairs_extra, dist_extra, n_water=40, seed=4401):
    """n_water good waters in front of the given atoms / constraints.  Returns the case and the index of the first extra atom."""
    case = instances('water', n_water, seed)
    base = len(case['x0'])
    pairs = np.vstack([case['pairs'], np.asarray(pairs_extra, dtype=np.int32).reshape(-1, 2) + base]).astype(np.int32)
    out = dict(x0=np.vstack([case['x0'], x_extra]), mass=np.concatenate([case['mass'], m_extra]), pairs=pairs,
               dist=np.concatenate([case['dist'], dist_extra]), free=case['free'], clusters=case['clusters'])
    return out, base


def perpendicular_pair():
    """A pair whose reference bond lies along x and whose current bond lies along y: the SHAKE update divides by r . p == 0.0.
    Returns (case, current positions, the two atoms)."""
    case, base = with_waters(np.array([[1.0, 1.0, 1.0], [1.1, 1.0, 1.0]]), [12.011, 1.008], [(0, 1)], [0.1])
    x = moved(case)
    x[base], x[base + 1] = [1.0, 1.0, 1.0], [1.0, 1.12, 1.0]
    return case, x, [base, base + 1]


def impossible_triangle(generic):
    """Sides 0.1 / 0.1 / 0.3 nm: no triangle has them.  generic: a fourth atom bound to the first makes it a 4-atom cluster of the
    generic class.  The positions are an equilateral triangle of side 0.1 nm.  Returns (case, the cluster's atoms)."""
    xs = [[2.0, 2.0, 2.0], [2.1, 2.0, 2.0], [2.05, 2.0 + 0.1 * np.sqrt(0.75), 2.0]]
    ms, pairs, dist = [12.011, 1.008, 3.5], [(0, 1), (0, 2), (1, 2)], [0.1, 0.1, 0.3]
    if generic:
        xs, ms, pairs, dist = xs + [[2.0, 2.0, 2.109]], ms + [1.008], pairs + [(0, 3)], dist + [0.109]
    case, base = with_waters(np.array(xs), ms, pairs, dist)
    return case, list(range(base, base + len(ms)))
