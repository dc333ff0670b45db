"""tests/drude_cases.py -- the cases of the DrudeForce tests, shared by the host and the GPU tests: the smallest that can still go
wrong.  TEST INFRASTRUCTURE ONLY.  A case is a dict: x [n][3], mass [n], rows (p, p1, p2, p3, p4, q, alpha, a12, a34), pairs (entry,
entry, thole), box (edges or None) and periodic.

  a         one isotropic pair
  b         one particle with p2 only, one with p3 / p4 only, one with all four, in a general (non-collinear) geometry
  c-*       two screened dipoles at thole 1.3 and 2.6, the Drude-Drude separation chosen for u = 0.05 .. 20
  d65, d129 65 and 129 Drude particles, 130 screened pairs between random neighbours (the lanes cross wavefront and block boundaries);
            every parent is the anchor (p2 .. p4) of other springs, so the gather sums more than one slot
  e65, e129 the same in a 2 nm box with periodic displacements, neighbours taken across the faces
(f, swm4_box(3) under PME, is built by the tests from atomsmm_amd.testing.)"""
import functools

import numpy as np

from atomsmm_amd import openmm

ALPHA = 1.0e-3          # nm^3: (alpha alpha)^(1/6) = 0.1 nm, so s = 10 thole / nm
C_THOLES = (1.3, 2.6)
C_US = (0.05, 0.3, 1.0, 3.0, 8.0, 20.0)


def case_a():
    x = np.array([[0.10, 0.20, 0.30], [0.112, 0.193, 0.305]])
    return dict(x=x, mass=np.array([15.6, 0.4]), rows=[(1, 0, -1, -1, -1, -1.7, 0.98e-3, 1.0, 1.0)], pairs=[], box=None, periodic=False)


def case_b():
    rng = np.random.default_rng(11)
    # three heavy-atom frames of five atoms each: parent, three anchors, the Drude particle
    x, mass, rows = [], [], []
    for k, (use2, use34) in enumerate([(True, False), (False, True), (True, True)]):
        base = len(x)
        origin = np.array([0.5 * k, 0.1 * k, -0.2 * k])
        x += [origin, origin + [0.12, 0.03, -0.02], origin + [-0.05, 0.11, 0.04], origin + [0.02, -0.06, 0.13],
              origin + rng.normal(scale=0.012, size=3)]
        mass += [12.0, 14.0, 16.0, 1.0, 0.4]
        rows.append((base + 4, base, base + 1 if use2 else -1, base + 2 if use34 else -1, base + 3 if use34 else -1,
                     -1.2 - 0.3 * k, (0.9 + 0.2 * k) * 1e-3, 0.8 + 0.1 * k, 1.15 - 0.1 * k))
    return dict(x=np.array(x), mass=np.array(mass), rows=rows, pairs=[], box=None, periodic=False)


def case_c(thole, u):
    """Two dipoles: parents 0 and 2, Drude particles 1 and 3; the Drude-Drude distance is u / s."""
    s = thole / (ALPHA * ALPHA) ** (1.0 / 6.0)
    r = u / s
    e = np.array([0.6, -0.48, 0.64])                      # a unit vector
    x = np.array([[0.0, 0.0, 0.0], [0.011, -0.006, 0.004], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    x[3] = x[1] + r * e
    x[2] = x[3] - np.array([-0.007, 0.009, 0.005])
    rows = [(1, 0, -1, -1, -1, -1.5, ALPHA, 1.0, 1.0), (3, 2, -1, -1, -1, -2.0, ALPHA, 1.0, 1.0)]
    return dict(x=x, mass=np.array([12.0, 0.4, 16.0, 0.4]), rows=rows, pairs=[(0, 1, thole)], box=None, periodic=False)


@functools.lru_cache(maxsize=None)
def _lattice(n_drude, periodic):
    """n_drude parents on a jittered lattice (6 x 6 a layer, spacing 1/3 nm, at most four layers), each with a Drude particle; atoms
    2 k (parent), 2 k + 1 (Drude).  Neighbours are lattice neighbours -- in x and y across the faces of the 2 nm box when periodic
    (the layers do not fill the box in z: there the neighbours are the raw ones)."""
    rng = np.random.default_rng(65 + n_drude + (1000 if periodic else 0))
    side, a = 6, 1.0 / 3.0
    layers = -(-n_drude // (side * side))
    assert layers <= 4
    cells = [(i, j, k) for k in range(layers) for j in range(side) for i in range(side)][:n_drude]
    index = {c: n for n, c in enumerate(cells)}
    box = np.array([2.0, 2.0, 2.0]) if periodic else None

    def neighbour(c, step):
        t = tuple(c[q] + step[q] for q in range(3))
        if periodic:
            t = (t[0] % side, t[1] % side, t[2])
        return index.get(t)
    parents = np.array(cells, dtype=float) * a + rng.normal(scale=0.03, size=(n_drude, 3)) + 0.01
    x = np.empty((2 * n_drude, 3))
    x[0::2] = parents
    x[1::2] = parents + rng.normal(scale=0.012, size=(n_drude, 3))
    if periodic:
        x[:, :2] = np.mod(x[:, :2], 2.0)       # (atoms that the jitter put outside come back through the opposite face)
    mass = np.empty(2 * n_drude)
    mass[0::2] = rng.choice([12.011, 14.007, 15.999], n_drude)
    mass[1::2] = 0.4
    steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    rows, pair_set = [], set()
    for n, c in enumerate(cells):
        near = [m for m in (neighbour(c, s) for s in steps) if m is not None and m != n]
        near = list(dict.fromkeys(near))
        rng.shuffle(near)
        kind = n % 4                                           # isotropic, p2 only, p3 / p4 only, all four
        p2 = 2 * near[0] if kind in (1, 3) and len(near) >= 1 else -1
        p3, p4 = (2 * near[1], 2 * near[2]) if kind in (2, 3) and len(near) >= 3 else (-1, -1)
        rows.append((2 * n + 1, 2 * n, p2, p3, p4, -1.0 - 0.01 * (n % 17), (0.8 + 0.01 * (n % 23)) * 1e-3, 0.7 + 0.02 * (n % 11),
                     1.2 - 0.02 * (n % 7)))
    candidates = sorted({(min(n, m), max(n, m)) for n, c in enumerate(cells) for s in steps for m in [neighbour(c, s)]
                         if m is not None and m != n})
    order = rng.permutation(len(candidates))[:130]
    pairs = [(candidates[k][0], candidates[k][1], float(rng.choice([1.3, 2.6]))) for k in sorted(order)]
    assert len(pairs) == 130
    return dict(x=x, mass=mass, rows=rows, pairs=pairs, box=box, periodic=periodic)


def case_d(n_drude):
    return _lattice(n_drude, False)


def case_e(n_drude):
    return _lattice(n_drude, True)


def small_cases():
    """name -> case for (a) to (e)."""
    cases = {'a': case_a(), 'b': case_b()}
    for thole in C_THOLES:
        for u in C_US:
            cases['c-%g-%g' % (thole, u)] = case_c(thole, u)
    for n in (65, 129):
        cases['d%d' % n] = case_d(n)
        cases['e%d' % n] = case_e(n)
    return cases


def force_of(case):
    force = openmm.DrudeForce()
    for row in case['rows']:
        force.addParticle(*row)
    for pair in case['pairs']:
        force.addScreenedPair(*pair)
    force.setUsesPeriodicBoundaryConditions(bool(case['periodic']))
    return force


def system_of(case, force=None):
    """A System with the case's masses (and box) and its DrudeForce; returns (system, force)."""
    system = openmm.System()
    for m in case['mass']:
        system.addParticle(float(m))
    if case['box'] is not None:
        L = case['box']
        system.setDefaultPeriodicBoxVectors((float(L[0]), 0, 0), (0, float(L[1]), 0), (0, 0, float(L[2])))
    force = force_of(case) if force is None else force
    system.addForce(force)
    return system, force
