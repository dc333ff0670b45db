"""GPU tests (run with -m gpu on an MI355X) of the SHAKE / RATTLE sweeps (csrc/cons_sweeps.h) where the rest of the suite does not go:
rigid clusters with cycles and clusters at the 8-atom / 16-constraint limits, scalene triangles in all 48 listings, atom numberings
that scatter every cluster through the index range, sets with empty and exactly full unit classes of k_stock (csrc/stock.hip),
re-created sets -- and the failure path: a cluster that is not finite or cannot converge is reported by amm_check, a refused set leaves
the previous one in force.  Through the C ABI on bare contexts: no force objects, no neighbour list; nothing but the solver reads the
positions.

The inputs are those of tests/constraint_cases.py; tests/test_constraint_cases_host.py holds the restatement (tests/stock_ref.py)
inside 350 of the 500 sweeps on every one of them.  Bounds: device against restatement as test_gpu_stock.py (positions 1e-12 nm,
velocities 1e-12/dt); against the exact solutions (oracle/constraints_oracle.py) at a tolerance of 1e-13, four times the distance of
the restatement itself from them on the same inputs (the kernel contracts into FMA what numpy rounds twice, over up to 278
sweeps), at least 1e-13 nm / 1e-11 nm/ps, the bounds of test_tight_tolerance_meets_the_exact_solutions."""
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from atomsmm_amd import backend as B  # noqa: E402
import constraint_cases as K  # noqa: E402
import stock_ref as SR  # noqa: E402
from test_gpu_stock import BOUND_V, BOUND_X  # noqa: E402

assert BOUND_V == BOUND_X / K.DT
EPS = np.finfo(np.float64).eps
SAVE_REF, CONSTRAIN_X, CONSTRAIN_V = (B.Op(op, 0, 0, 0, 0.0) for op in (B.OP_SAVE_REF, B.OP_CONSTRAIN_X, B.OP_CONSTRAIN_V))
NOT_CONVERGED = 'did not converge'


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


class Bare:
    """A context with a state and (pairs given) a constraint set; f: a force buffer in slot 0."""

    def __init__(self, case, tol=1e-5, x=None, v=None, f=None, constrained=True):
        n = len(case['x0'])
        self.ctx = B.HipContext(n, np.array([K.BOX] * 3))
        self.x, self.v = dev(case['x0'] if x is None else x), dev(np.zeros((n, 3)) if v is None else v)
        self.ctx.bind_state(self.x, self.v, dev(case['mass']))
        if f is not None:
            self.f = dev(f)
            self.ctx.bind_buffer(0, self.f)
        if constrained:
            self.ctx.constraints_create(case['pairs'], case['dist'], tol)
        self.ctx.expr_seed(K.SEED)

    def stock(self, kind, steps=1, check=True):
        sid = self.ctx.stock_define(kind, K.DT, K.FRICTION[kind], K.KT)
        self.ctx.run_ops([B.Op(B.OP_STOCK, sid, 0, 0, 0.0)], steps)
        if check:
            self.ctx.check()
        return self.state()

    def run(self, *ops, check=True):
        self.ctx.run_ops(list(ops), 1)
        if check:
            self.ctx.check()
        return self.state()

    def state(self):
        return self.x.cpu().numpy(), self.v.cpu().numpy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def solvers_on_device(case, tol, xin, vin):
    """SAVE_REF at x0 ; x = xin ; CONSTRAIN_X ; CONSTRAIN_V"""
    with Bare(case, tol, v=vin) as c:
        c.run(SAVE_REF)
        c.x.copy_(dev(xin))
        return c.run(CONSTRAIN_X, CONSTRAIN_V)


def close_to(got, want, what):
    dx, dv = np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()
    print('%s: max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e nm/ps (bound %.0e)' % (what, dx, BOUND_X, dv, BOUND_V))
    assert dx < BOUND_X and dv < BOUND_V, what


def satisfied(case, x, tol):
    i, j = case['pairs'].T
    assert (np.abs(np.linalg.norm(x[i] - x[j], axis=1) / case['dist'] - 1) < 1.01 * tol + 5e-14).all()


def against_the_oracle(case, xin, xref, got, want, vin=None):
    """Bound: 4 x the restatement's own distance from the exact solutions per shape, at least 1e-13 nm / 1e-11 nm/ps."""
    ours = K.oracle_distances(case, xin, xref, got[0], vin, got[1] if vin is not None else None)
    theirs = K.oracle_distances(case, xin, xref, want[0], vin, want[1] if vin is not None else None)
    for name in ours:
        bx, bv = max(4 * theirs[name][0], 1e-13), max(4 * theirs[name][1], 1e-11)
        print('%-8s - oracle: kernel %.1e nm, %.1e nm/ps; restatement %.1e nm, %.1e nm/ps' % (name, *ours[name], *theirs[name]))
        assert ours[name][0] < bx and ours[name][1] < bv, name
    assert 'methane' not in ours


# ------------------------------------------------------------------------------------ rigid shapes, plain and scattered numbering
LAYOUTS = {'plain': lambda: (K.mixed(), None), 'scattered': K.mixed_scattered}


@functools.lru_cache(maxsize=None)
def mixed_inputs(layout):
    case, perm = LAYOUTS[layout]()
    xin, vin = K.moved(K.mixed()), K.velocities(K.mixed())
    v, f = K.thermal(K.mixed())
    if perm is not None:
        xin, vin, v, f = (scattered_like(a, perm) for a in (xin, vin, v, f))
    return case, perm, xin, vin, v, f


def scattered_like(a, perm):
    out = np.empty_like(a)
    out[perm] = a
    return out


@functools.lru_cache(maxsize=None)
def mixed_solved(layout, tol):
    """(device result, restatement) of the stand-alone solvers on the mixed set, each computed once."""
    case, _, xin, vin, _, _ = mixed_inputs(layout)
    want = K.restated_solvers(case, tol, xin, vin)
    assert max(want[2:]) <= K.CAP
    return solvers_on_device(case, tol, xin, vin), want[:2]


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
@pytest.mark.parametrize('layout', ['plain', 'scattered'])
def test_rigid_shapes_through_the_solvers(layout, tol):
    """16 methyls (6 constraints on 4 atoms), methanes (10 on 5, one redundant), puckered six-rings (12 on 6) and eight-rings (16 on 8:
    both limits of a cluster), the 48 scalene listings, 30 waters and 17 free atoms through k_shake / k_rattle; `scattered`: the
    same set with its atoms renumbered at random and its constraint list shuffled."""
    case, _, xin, vin, _, _ = mixed_inputs(layout)
    got, want = mixed_solved(layout, tol)
    close_to(got, want, 'solvers')                                                        # (a) the restatement
    satisfied(case, got[0], tol)                                                          # (b) the constraints
    i, j = case['pairs'].T
    dp, dw = got[0][i] - got[0][j], got[1][i] - got[1][j]
    # (c) no relative velocity along a constraint: the RATTLE criterion |dp . dw| <= tol |dp|^2, with the rounding of a 3-term dot product
    assert (np.abs((dp * dw).sum(1)) <= 1.01 * tol * (dp * dp).sum(1) + 8 * EPS * (np.abs(dp) * np.abs(dw)).sum(1)).all()
    for _, atoms, _, _ in case['clusters']:
        m = case['mass'][atoms, None]
        assert np.abs((m * (got[0][atoms] - xin[atoms])).sum(0) / m.sum()).max() < 1e-12            # ... and each centre of mass stays
    if tol == 1e-13:
        against_the_oracle(case, xin, case['x0'], got, want, vin)                         # (d) the exact solutions
    free = case['free']
    assert len(free) == 17 and np.array_equal(got[0][free], xin[free]) and np.array_equal(got[1][free], vin[free])      # (e)


@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE, SR.LANGEVIN, SR.BROWNIAN])
@pytest.mark.parametrize('layout', ['plain', 'scattered'])
def test_rigid_shapes_through_the_stock_step(layout, kind):
    """The mixed set through AMM_OP_STOCK: the rigid shapes take the generic path of k_stock<true>, the triangles the fixed one."""
    case, _, _, _, v, f = mixed_inputs(layout)
    states, worst = K.restated_steps(case, kind, 1e-5, v=v, f=f)
    assert worst <= K.CAP
    with Bare(case, 1e-5, v=v, f=f) as c:
        close_to(c.stock(kind), states[0], 'step 1')
        last = c.stock(kind, K.STEPS - 1)
        close_to(last, states[-1], 'step %d' % K.STEPS)
        satisfied(case, last[0], 1e-5)


@functools.lru_cache(maxsize=None)
def verlet_step_on_device(layout):
    case, _, _, _, v, f = mixed_inputs(layout)
    with Bare(case, 1e-5, v=v, f=f) as c:
        return c.stock(SR.VERLET)


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
def test_the_numbering_of_the_atoms_does_not_reach_the_bits(tol):
    """Equivariance: the run on the scattered set, un-permuted, equals the run on the plain set bit for bit -- CONSTRAIN_X, CONSTRAIN_V
    and a Verlet step (which draws no random numbers; the Langevin kinds index their Gaussians by atom).  The sweeps visit a cluster's
    constraints in listing order and every update is symmetric in i and j (cons_sweeps.h)."""
    perm = K.mixed_scattered()[1]
    (xa, va), _ = mixed_solved('plain', tol)
    (xb, vb), _ = mixed_solved('scattered', tol)
    assert np.array_equal(xb[perm], xa), 'CONSTRAIN_X'
    assert np.array_equal(vb[perm], va), 'CONSTRAIN_V'
    xa, va = verlet_step_on_device('plain')
    xb, vb = verlet_step_on_device('scattered')
    assert np.array_equal(xb[perm], xa) and np.array_equal(vb[perm], va), 'OP_STOCK'


# ------------------------------------------------------------------------------------ the triangle fast path
@pytest.mark.parametrize('tol', [1e-5, 1e-13])
@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE])
def test_scalene_triangles_through_the_stock_step(kind, tol):
    """A triangle with three different sides and three different masses in all 6 orders of its constraints x 8 orientations, and 16
    waters: amm_constraints_create_impl classes all 64 as triangles (three atoms, three constraints that close), so that k_stock
    solves them with ConsShapeTriangle from the atoms in d_fixed -- where isosceles water with two equal masses cannot tell two
    entries of d_fixed or of the distances apart."""
    case = K.triangles()
    cl = K.clusters_of(case)
    assert [(len(idx), len(local)) for idx, local, _ in cl.list] == [(3, 3)] * 64 and cl.constrained.all()
    states, worst = K.restated_steps(case, kind, tol)
    assert worst <= K.CAP
    v, f = K.thermal(case)
    with Bare(case, tol, v=v, f=f) as c:
        first = c.stock(kind)
        close_to(first, states[0], 'step 1')
        last = c.stock(kind, K.STEPS - 1)
        close_to(last, states[-1], 'step %d' % K.STEPS)
        satisfied(case, last[0], tol)
    if kind == SR.VERLET and tol == 1e-13:
        x1 = case['x0'] + K.DT * (v + (K.DT * f) / case['mass'][:, None])
        against_the_oracle(case, x1, case['x0'], first, states[0])


# ------------------------------------------------------------------------------------ the unit classes of k_stock
@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE])
@pytest.mark.parametrize('n_tri, n_two, n_gen, n_free', [(64, 0, 0, 0), (0, 64, 0, 1), (0, 0, 1, 0), (0, 0, 0, 5), (128, 64, 64, 0),
                                                         (1, 1, 1, 1), (65, 63, 2, 129)])
def test_class_census_of_the_stock_step(n_tri, n_two, n_gen, n_free, kind):
    """Triangles, pairs, other clusters and free atoms each start at a multiple of 64 in k_stock's unit index space: empty classes,
    classes of exactly 64 and 128 units, a total of exactly 256 (one full block), one unit of each, one past and one short of 64.
    (0, 0, 0, 5) is a set created with no constraint at all."""
    case = K.census(n_tri, n_two, n_gen, n_free)
    cl = K.clusters_of(case)
    shapes = [(len(idx), len(local)) for idx, local, _ in cl.list]
    assert (shapes.count((3, 3)), shapes.count((2, 1)), int((~cl.constrained).sum())) == (n_tri, n_two, n_free)
    assert len(shapes) == n_tri + n_two + n_gen and (len(shapes) > 0 or len(case['pairs']) == 0)
    states, worst = K.restated_steps(case, kind, 1e-5)
    assert worst <= K.CAP
    v, f = K.thermal(case)
    with Bare(case, 1e-5, v=v, f=f) as c:
        close_to(c.stock(kind), states[0], 'step 1')
        last = c.stock(kind, K.STEPS - 1)
        close_to(last, states[-1], 'step %d' % K.STEPS)
        satisfied(case, last[0], 1e-5)
        # the step left its positions as the solver's reference, for every class: a CONSTRAIN_X without SAVE_REF shakes along them
        xin = last[0] + np.random.default_rng(5).normal(0.0, 0.002, last[0].shape)
        c.x.copy_(dev(xin))
        want, sweeps = SR.shake(xin, last[0], case['mass'], cl, 1e-5)
        assert sweeps <= K.CAP
        assert np.abs(c.run(CONSTRAIN_X)[0] - want).max() < BOUND_X


# ------------------------------------------------------------------------------------ a second set in one context
def methyls_two_ways():
    """30 methyls; set A constrains each one's three hydrogens (a triangle, the carbon free), set B the whole group (generic)."""
    full = K.instances('methyl', 30, 4501)
    keep = np.array([q for q, (i, j) in enumerate(full['pairs']) if i % 4 and j % 4])
    return dict(full, pairs=full['pairs'][keep], dist=full['dist'][keep]), full


def test_a_second_set_replaces_the_first():
    """Create A and step, create B over the same atoms and step: as a fresh context with B alone, bit for bit."""
    a, b = methyls_two_ways()
    assert {(len(i), len(l)) for i, l, _ in K.clusters_of(a).list} == {(3, 3)} and {(len(i), len(l)) for i, l, _ in K.clusters_of(b).list} == {(4, 6)}
    v, f = K.thermal(b)
    xin = K.moved(b)
    with Bare(a, 1e-5, v=v, f=f) as c:
        xa, va = c.stock(SR.VERLET)
        assert np.abs(xa - a['x0']).max() > 1e-4
        c.ctx.constraints_create(b['pairs'], b['dist'], 1e-7)
        after = [c.stock(SR.VERLET), c.run(CONSTRAIN_V)]
        c.x.copy_(dev(xin))
        after.append(c.run(CONSTRAIN_X))            # (no SAVE_REF: along the positions the step left)
    with Bare(b, 1e-7, x=xa, v=va, f=f) as c:
        fresh = [c.stock(SR.VERLET), c.run(CONSTRAIN_V)]
        c.x.copy_(dev(xin))
        fresh.append(c.run(CONSTRAIN_X))
    for (x1, v1), (x2, v2) in zip(after, fresh):
        assert np.array_equal(x1, x2) and np.array_equal(v1, v2)
    x1, v1, sweeps = SR.step(SR.VERLET, xa, va, f, b['mass'], K.clusters_of(b), K.DT, 0.0, K.KT, 1e-7, K.SEED, 1)
    assert sweeps <= K.CAP
    close_to(after[0], (x1, v1), 'the step under set B')
    satisfied(b, after[0][0], 1e-7)
    satisfied(b, after[2][0], 1e-7)
    assert np.abs(after[2][0] - xin).max() > 1e-4


@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE])
def test_a_set_of_no_constraints(kind):
    """n_constraints = 0, as a first set and in place of a real one: the three constraint ops are identities, the stock step is that
    of a context without a set."""
    a, _ = methyls_two_ways()
    none = dict(a, pairs=np.zeros((0, 2), dtype=np.int32), dist=np.zeros(0))
    v, f = K.thermal(a)
    xin = K.moved(a)
    with Bare(a, constrained=False, x=xin, v=v, f=f) as c:
        want = c.stock(kind, K.STEPS)
    for first in (none, a):
        with Bare(first, x=xin, v=v, f=f) as c:
            c.ctx.constraints_create(none['pairs'], none['dist'], 1e-5)
            got = c.run(SAVE_REF, CONSTRAIN_X, CONSTRAIN_V)
            assert np.array_equal(got[0], xin) and np.array_equal(got[1], v)
            got = c.stock(kind, K.STEPS)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.abs(want[0] - xin).max() > 1e-4


# ------------------------------------------------------------------------------------ failures
def raises_not_converged(c):
    with pytest.raises(B.HipError, match=NOT_CONVERGED):
        c.ctx.check()
    c.ctx.check()                # the flag is cleared by the call that reports it


def rest_as_restated(case, bad, got, xin, xref, tol=1e-5):
    """Every cluster but the bad one: finite and as the restatement has it."""
    rest = np.setdiff1d(np.arange(len(xin)), bad)
    with np.errstate(all='ignore'):
        want, _ = SR.shake(xin, xref, case['mass'], K.clusters_of(case), tol)
    assert np.isfinite(got[rest]).all() and np.abs(got[rest] - want[rest]).max() < BOUND_X


def test_a_perpendicular_pair_is_reported():
    """The reference bond along x, the current bond along y: r . p == 0.0 exactly, the update is +-inf along the reference bond and NaN
    across it, and every later sweep sees |p|^2 = NaN.  (With `pp < lower*d2 || pp > upper*d2` as the test for "not there yet" that
    sweep found nothing to do and the cluster counted as converged: amm_check passed with NaN in x.)"""
    case, xin, bad = K.perpendicular_pair()
    with Bare(case) as c:
        c.run(SAVE_REF)
        c.x.copy_(dev(xin))
        got, _ = c.run(CONSTRAIN_X, check=False)
        raises_not_converged(c)
        rest_as_restated(case, bad, got, xin, case['x0'])
        # the atoms put back: the set is whole again
        xin[bad] = case['x0'][bad] + [[0.0, 0.0, 0.0], [0.0, 0.004, 0.0]]
        c.x.copy_(dev(case['x0']))
        c.run(SAVE_REF)
        c.x.copy_(dev(xin))
        got, _ = c.run(CONSTRAIN_X)
        satisfied(case, got, 1e-5)
        assert np.abs(got - SR.shake(xin, case['x0'], case['mass'], K.clusters_of(case), 1e-5)[0]).max() < BOUND_X


@pytest.mark.parametrize('where', [0, 1, 2])
def test_nan_is_reported_by_the_solvers(where):
    """NaN in one coordinate / one velocity component of a triangle, a pair or a generic cluster (a force blow-up leaves such)."""
    case = K.census(3, 2, 2, 1)
    atoms = [a for name, a, _, _ in case['clusters'] if (name in ('scalene', 'water'), name == 'pair', name in ('xh3', 'methyl'))[where]][0]
    xin, vin = K.moved(case), K.velocities(case)
    with Bare(case, v=vin) as c:
        c.run(SAVE_REF)
        bad = xin.copy()
        bad[atoms[-1], 1] = np.nan
        c.x.copy_(dev(bad))
        got, _ = c.run(CONSTRAIN_X, check=False)
        raises_not_converged(c)
        rest_as_restated(case, atoms, got, bad, case['x0'])
        c.x.copy_(dev(case['x0']))
        c.run(SAVE_REF, CONSTRAIN_X, CONSTRAIN_V)          # clean again
        bad = vin.copy()
        bad[atoms[0], 2] = np.nan
        c.v.copy_(dev(bad))
        c.run(CONSTRAIN_V, check=False)
        raises_not_converged(c)


@pytest.mark.parametrize('broken', ['x', 'v'])
@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE])
@pytest.mark.parametrize('where', [0, 1, 2])
def test_nan_is_reported_by_the_stock_step(where, kind, broken):
    case = K.census(3, 2, 2, 1)
    atoms = [a for name, a, _, _ in case['clusters'] if (name in ('scalene', 'water'), name == 'pair', name in ('xh3', 'methyl'))[where]][0]
    v, f = K.thermal(case)
    x = case['x0'].copy()
    (x if broken == 'x' else v)[atoms[0], 0] = np.nan
    with Bare(case, x=x, v=v, f=f) as c:
        got, _ = c.stock(kind, check=False)
        raises_not_converged(c)
        rest = np.setdiff1d(np.arange(len(x)), atoms)
        with np.errstate(all='ignore'):
            want = K.restated_steps(dict(case, x0=x), kind, 1e-5, steps=1, v=v, f=f)[0][0][0]
        assert np.isfinite(got[rest]).all() and np.abs(got[rest] - want[rest]).max() < BOUND_X


@pytest.mark.parametrize('generic', [False, True])
def test_distances_no_triangle_has_are_reported(generic):
    """Sides 0.1 / 0.1 / 0.3 nm, as a cluster of the triangle class and inside a 4-atom cluster of the generic class: the sweeps stay
    finite and have nothing to converge to."""
    case, bad = K.impossible_triangle(generic)
    xin = K.moved(case)
    with Bare(case) as c:
        c.run(SAVE_REF)
        c.x.copy_(dev(xin))
        got, _ = c.run(CONSTRAIN_X, check=False)
        raises_not_converged(c)
        rest_as_restated(case, bad, got, xin, case['x0'])
    v, f = K.thermal(case)
    for kind in (SR.VERLET, SR.LANGEVIN_MIDDLE):
        with Bare(case, v=v, f=f) as c:
            c.stock(kind, check=False)
            raises_not_converged(c)


def refused_sets(n):
    """(pairs, distances, the library's text) of sets amm_constraints_create must refuse in a context of n >= 9 atoms."""
    limit, bad = 'exceeds 8 atoms / 16 constraints', 'bad constraint'
    eight = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    assert len(eight[:17]) == 17 and {a for p in eight[:17] for a in p} <= set(range(8))
    yield [(k, k + 1) for k in range(8)], [0.15] * 8, limit                  # a chain of 9 atoms
    yield eight[:17], [0.15] * 17, limit                                     # 17 constraints among atoms 0 .. 7
    yield eight[:16] + [(2, 3)], [0.15] * 17, limit                          # ... the 17th a repetition
    for pair in ((3, 3), (-1, 2), (2, -1), (n, 0), (0, n)):
        yield [(0, 1), pair], [0.1, 0.1], bad
    for d in (0.0, -0.1, np.nan):
        yield [(0, 1), (1, 2)], [0.1, d], bad


def test_sets_that_are_refused():
    case = K.instances('water', 4, 1)
    with Bare(case, constrained=False) as c:
        for pairs, dist, text in refused_sets(len(case['x0'])):
            with pytest.raises(B.HipError, match=re.escape(text)):
                c.ctx.constraints_create(np.array(pairs, dtype=np.int32), np.array(dist), 1e-5)
        # at the limits: 8 atoms, 16 constraints
        eight = [(i, j) for i in range(8) for j in range(i + 1, 8)][:16]
        c.ctx.constraints_create(np.array(eight, dtype=np.int32), np.full(16, 0.15), 1e-5)
        c.ctx.check()


def test_a_refused_set_leaves_the_previous_one_in_force():
    """(amm_constraints_create used to free the old set before it looked at the new one: after a refusal the context had no set at
    all, and CONSTRAIN_X / CONSTRAIN_V were identities.)"""
    case = K.instances('water', 40, 4601)
    xin, vin = K.moved(case), K.velocities(case)
    want = K.restated_solvers(case, 1e-7, xin, vin)
    with Bare(case, 1e-7, v=vin) as c:
        for pairs, dist, text in list(refused_sets(len(xin)))[::3]:
            with pytest.raises(B.HipError, match=re.escape(text)):
                c.ctx.constraints_create(np.array(pairs, dtype=np.int32), np.array(dist), 1e-5)
        c.run(SAVE_REF)
        c.x.copy_(dev(xin))
        got = c.run(CONSTRAIN_X, CONSTRAIN_V)
        assert np.abs(got[0] - xin).max() > 1e-4
        satisfied(case, got[0], 1e-7)                # (the old set with its own tolerance)
        close_to(got, want[:2], 'after a refused set')
