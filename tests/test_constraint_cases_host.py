"""CPU tests of the constraint cases (tests/constraint_cases.py) and of the restatement of the solvers (tests/stock_ref.py) on them:
the conditions the GPU tests (test_gpu_constraint_shapes.py) rest on, stated on the reference alone.

  * the restatement converges well inside the 500 sweeps on every committed input (at most 350), so that no GPU test sits on the cap;
  * at a tolerance of 1e-13 it lands on the exact solutions of the constraint equations (oracle/constraints_oracle.py);
  * renumbering the atoms and shuffling the constraint list change neither the clusters nor one bit of its results;
  * on the inputs on which the solvers must fail -- a division by zero, NaN, distances no triangle has -- it reports failure.

Sweeps the restatement used here (30 instances per shape, sigma = 0.003 nm; SHAKE / RATTLE):
    shape      tol 1e-5     tol 1e-13
    methyl      49 / 76     154 / 182
    methane     19 / 28      53 / 64
    ring6       64 / 110    234 / 278
    ring8       32 / 51      98 / 120
    scalene      9 / 13      22 / 26
    water       18 / 29      54 / 65       (trees: pair 5 / 2, X-H3 9 / 10, 8-atom chain 44 / 53 at 1e-13)
and its largest distance from the exact solutions at 1e-13: positions 6.7e-14 nm, velocities 6.4e-14 nm/ps (ring6; methyl 3.3e-14 /
2.9e-14, ring8 3.1e-14 / 2.8e-14, scalene 2.0e-14 / 2.0e-14)."""
import numpy as np
import pytest

import constraint_cases as K
import stock_ref as SR

COUNT = 30


def per_shape(name):
    return K.instances(name, 48 if name == 'scalene' else COUNT, 5000 + (K.RIGID + K.KNOWN).index(name))


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
@pytest.mark.parametrize('name', K.RIGID + K.KNOWN)
def test_the_restatement_stays_inside_the_sweep_cap(name, tol):
    case = per_shape(name)
    _, _, ns, nr = K.restated_solvers(case, tol)
    print('%s at %.0e: SHAKE %d sweeps, RATTLE %d' % (name, tol, ns, nr))
    assert 1 <= ns <= K.CAP and 1 <= nr <= K.CAP


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
def test_the_sets_of_the_gpu_tests_stay_inside_the_sweep_cap(tol):
    """The very inputs of test_gpu_constraint_shapes.py: the mixed set through the solvers, and through three steps of each stock kind
    at the tolerance they run at there; the triangles through Verlet and LangevinMiddle."""
    ns, nr = K.restated_solvers(K.mixed(), tol)[2:]
    worst = {'solvers': max(ns, nr)}
    for kind in (SR.VERLET, SR.LANGEVIN_MIDDLE):
        worst['triangles %d' % kind] = K.restated_steps(K.triangles(), kind, tol)[1]
    if tol == 1e-5:
        scattered, perm = K.mixed_scattered()
        v, f = (np.empty_like(a) for a in K.thermal(K.mixed()))
        v[perm], f[perm] = K.thermal(K.mixed())
        for kind in (SR.VERLET, SR.LANGEVIN_MIDDLE, SR.LANGEVIN, SR.BROWNIAN):
            worst['mixed %d' % kind] = K.restated_steps(K.mixed(), kind, tol)[1]
            worst['scattered %d' % kind] = K.restated_steps(scattered, kind, tol, v=v, f=f)[1]      # (other Gaussians: they go by atom)
    print(worst)
    assert max(worst.values()) <= K.CAP


def test_the_restatement_meets_the_exact_solutions():
    """Tolerance 1e-13, every shape but methane (ten constraints on nine internal coordinates: the Jacobian of Newton's method is
    singular).  The bounds are those of test_tight_tolerance_meets_the_exact_solutions; the GPU test takes four times the
    distances found here, on its own inputs, as the kernel's bound."""
    for name in [s for s in K.RIGID + K.KNOWN if s != 'methane']:
        case = per_shape(name)
        xin, vin = K.moved(case), K.velocities(case)
        xs, vs, _, _ = K.restated_solvers(case, 1e-13)
        (dx, dv), = K.oracle_distances(case, xin, case['x0'], xs, vin, vs).values()
        print('%-8s restatement - oracle: %.1e nm, %.1e nm/ps' % (name, dx, dv))
        assert dx < 1e-13 and dv < 1e-11, name


def test_methane_is_checked_by_its_constraints():
    case = per_shape('methane')
    xs, vs, _, _ = K.restated_solvers(case, 1e-13)
    i, j = case['pairs'].T
    assert np.abs(np.linalg.norm(xs[i] - xs[j], axis=1) / case['dist'] - 1).max() < 1.01e-13 + 5e-14
    dp = xs[i] - xs[j]
    assert (np.abs((dp * (vs[i] - vs[j])).sum(1)) <= 1.01e-13 * (dp * dp).sum(1) + 1e-16).all()


def test_every_set_is_consistent_and_seeded():
    for case in (K.mixed(), K.triangles(), K.census(65, 63, 2, 129), K.mixed_scattered()[0]):
        i, j = case['pairs'].T
        assert np.array_equal(np.linalg.norm(case['x0'][i] - case['x0'][j], axis=1), case['dist'])
        for name, atoms, local, dist in case['clusters']:
            assert len(atoms) <= 8 and len(local) <= 16
            assert np.allclose([np.linalg.norm(case['x0'][atoms[a]] - case['x0'][atoms[b]]) for a, b in local], dist, rtol=0, atol=1e-15)
    again = K.shuffled({'methyl': 3, 'ring8': 2, 'free': 4}, 9), K.shuffled({'methyl': 3, 'ring8': 2, 'free': 4}, 9)
    assert np.array_equal(again[0]['x0'], again[1]['x0']) and np.array_equal(again[0]['pairs'], again[1]['pairs'])
    shapes = sorted((len(atoms), len(local)) for _, atoms, local, _ in K.mixed()['clusters'])
    assert shapes == sorted([(4, 6)] * 16 + [(5, 10)] * 16 + [(6, 12)] * 16 + [(8, 16)] * 16 + [(3, 3)] * 78)
    # the 48 listings of the scalene triangle are 48 different ones, and every side has its own length and every corner its own mass
    listings = {tuple(local) for name, _, local, _ in K.triangles()['clusters'] if name == 'scalene'}
    assert len(listings) == 48
    _, atoms, local, dist = next(c for c in K.triangles()['clusters'] if c[0] == 'scalene')[0:4]
    assert len({round(d, 6) for d in dist}) == 3 and len(set(K.triangles()['mass'][atoms])) == 3


def shape_census(case):
    cl = K.clusters_of(case)
    return sorted((len(idx), len(local)) for idx, local, _ in cl.list), int((~cl.constrained).sum())


def test_scatter_and_interleave_keep_the_clusters_and_every_bit():
    plain = K.mixed()
    scattered, perm = K.mixed_scattered()
    assert shape_census(plain) == shape_census(scattered) == shape_census(K.scatter(plain, 1)[0]) == shape_census(K.interleave_constraints(plain, 2))
    assert sorted(perm) == list(range(len(perm)))
    # the clusters really are spread out, and the constraint list really is interleaved
    spans = [max(atoms) - min(atoms) for _, atoms, _, _ in scattered['clusters']]
    assert np.median(spans) > len(perm) // 3
    owner = {a: c for c, (_, atoms, _, _) in enumerate(scattered['clusters']) for a in atoms}
    listed = [owner[int(i)] for i, _ in scattered['pairs']]
    assert sum(a != b for a, b in zip(listed, listed[1:])) > 0.9 * len(listed)
    # ... and each cluster's constraints kept their order and orientation
    cl = K.clusters_of(scattered)
    by_first = {tuple(sorted(atoms)): (atoms, local) for _, atoms, local, _ in scattered['clusters']}
    for idx, local, _ in cl.list:
        atoms, listing = by_first[tuple(idx)]
        assert [(idx[a], idx[b]) for a, b in local] == [(atoms[a], atoms[b]) for a, b in listing]
    for tol in (1e-5, 1e-13):
        xs, vs, _, _ = K.restated_solvers(plain, tol)
        xin, vin = np.empty_like(xs), np.empty_like(vs)
        xin[perm], vin[perm] = K.moved(plain), K.velocities(plain)
        xp, vp, _, _ = K.restated_solvers(scattered, tol, xin, vin)
        assert np.array_equal(xp[perm], xs) and np.array_equal(vp[perm], vs)
        if tol == 1e-5:
            # the batches stock_ref.Clusters forms itself (by the atoms' rank in the numbering: nearly one per cluster here)
            own = K.clusters_of(scattered, regroup=False)
            assert len(own.batches) > 4 * len(cl.batches)
            xo, _ = SR.shake(xin, scattered['x0'], scattered['mass'], own, tol)
            vo, _ = SR.rattle(xo, vin, scattered['mass'], own, tol)
            assert np.array_equal(xo, xp) and np.array_equal(vo, vp)
    v, f = K.thermal(plain)
    vq, fq = np.empty_like(v), np.empty_like(f)
    vq[perm], fq[perm] = v, f
    a, _ = K.restated_steps(plain, SR.VERLET, 1e-5)
    b, _ = K.restated_steps(scattered, SR.VERLET, 1e-5, v=vq, f=fq)
    assert np.array_equal(b[-1][0][perm], a[-1][0]) and np.array_equal(b[-1][1][perm], a[-1][1])


@pytest.mark.parametrize('n_tri, n_two, n_gen, n_free', [(64, 0, 0, 0), (0, 64, 0, 1), (0, 0, 1, 0), (128, 64, 64, 0), (1, 1, 1, 1), (65, 63, 2, 129)])
def test_census_sets_have_the_classes_they_name(n_tri, n_two, n_gen, n_free):
    shapes, free = shape_census(K.census(n_tri, n_two, n_gen, n_free))
    assert shapes.count((3, 3)) == n_tri and shapes.count((2, 1)) == n_two and len(shapes) == n_tri + n_two + n_gen and free == n_free
    for kind in (SR.VERLET, SR.LANGEVIN_MIDDLE):
        assert K.restated_steps(K.census(n_tri, n_two, n_gen, n_free), kind, 1e-5)[1] <= K.CAP


# ------------------------------------------------------------------------------------ failures
def failed_only(case, x, xref, atoms, tol=1e-5):
    """SHAKE of the whole set: the cluster of `atoms` runs out of sweeps, every other one converges."""
    with np.errstate(all='ignore'):
        out, worst = SR.shake(x, xref, case['mass'], K.clusters_of(case), tol)
    rest = np.setdiff1d(np.arange(len(x)), atoms)
    good = dict(case, pairs=case['pairs'][np.isin(case['pairs'][:, 0], rest)], dist=case['dist'][np.isin(case['pairs'][:, 0], rest)])
    want, sweeps = SR.shake(x, xref, case['mass'], K.clusters_of(good), tol)
    assert worst == SR.SWEEPS + 1 and sweeps <= K.CAP
    assert np.array_equal(out[rest], want[rest]) and np.isfinite(out[rest]).all()
    return out


def test_a_perpendicular_pair_fails():
    case, x, atoms = K.perpendicular_pair()
    dr, dp = case['x0'][atoms[0]] - case['x0'][atoms[1]], x[atoms[0]] - x[atoms[1]]
    assert dr @ dp == 0.0 and abs(dp @ dp - 0.01) > 1e-3
    out = failed_only(case, x, case['x0'], atoms)
    assert not np.isfinite(out[atoms]).all()            # +-inf along the reference bond, NaN across it


def test_nan_fails():
    case = K.census(3, 2, 2, 1)
    cl = K.clusters_of(case)
    for name, atoms, _, _ in case['clusters']:
        x = K.moved(case)
        x[atoms[-1], 1] = np.nan
        failed_only(case, x, case['x0'], atoms)
        v = K.velocities(case)
        v[atoms[0], 2] = np.nan
        with np.errstate(all='ignore'):
            assert SR.rattle(case['x0'], v, case['mass'], cl, 1e-5)[1] == SR.SWEEPS + 1
    for kind, bad in ((SR.VERLET, 'x'), (SR.VERLET, 'v'), (SR.LANGEVIN_MIDDLE, 'x'), (SR.LANGEVIN_MIDDLE, 'v')):
        v, f = K.thermal(case)
        broken = dict(case, x0=case['x0'].copy())
        (broken['x0'] if bad == 'x' else v)[case['clusters'][0][1][0], 0] = np.nan
        with np.errstate(all='ignore'):
            assert K.restated_steps(broken, kind, 1e-5, steps=1, v=v)[1] == SR.SWEEPS + 1


@pytest.mark.parametrize('generic', [False, True])
def test_an_impossible_triangle_fails_and_stays_finite(generic):
    case, atoms = K.impossible_triangle(generic)
    shapes, _ = shape_census(case)
    assert shapes.count((4, 4) if generic else (3, 3)) == (1 if generic else 41)
    out = failed_only(case, K.moved(case), case['x0'], atoms)
    assert np.isfinite(out[atoms]).all()        # (it wanders: the sweeps have no fixed point to settle on)
    v, f = K.thermal(case)
    for kind in (SR.VERLET, SR.LANGEVIN_MIDDLE):
        states, worst = K.restated_steps(case, kind, 1e-5, steps=1)
        assert worst == SR.SWEEPS + 1 and np.isfinite(states[0][0]).all() and np.isfinite(states[0][1]).all()


def test_finite_inputs_see_the_predicates_they_always_saw():
    """The NaN-aware predicates ~(a <= x <= b), ~(|d| <= t) are the old ones (x < a | x > b), (|d| > t) on everything but NaN."""
    pp = np.array([0.0, 0.5, 1.0 - 1e-16, 1.0, 1.0 + 1e-16, 2.0, np.inf, -np.inf])
    for lower, upper in ((1.0, 1.0), (0.5, 2.0), (1.0 - 1e-16, 1.0 + 1e-16)):
        assert np.array_equal(~((pp >= lower) & (pp <= upper)), (pp < lower) | (pp > upper))
    assert np.array_equal(~(np.abs(pp - 1.0) <= 0.5), np.abs(pp - 1.0) > 0.5)
    assert (~((np.nan >= pp) & (np.nan <= pp))).all()
