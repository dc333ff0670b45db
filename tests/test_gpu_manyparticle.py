"""GPU tests of the many-particle force (csrc/manyparticle.hip): CustomManyParticleForce over sets of three with any energy text -- a
neighbour scan per particle, then one wavefront per particle that enumerates the sets it belongs to, queues the survivors in LDS for
the interpreter and keeps the force on its own particle.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|, 1e-12 nm for the short
trajectories.  References: tests/manyparticle_cases.py (the sets enumerated on the host in fp64 by the rules of DESIGN.md 3.MP; each
set a bond of three particles at 50 digits, forces by mpmath.diff in the atoms' own coordinates) on n = 3, 4, 6, and everywhere a
CustomCompoundBondForce that holds every host-enumerated set as an explicit bond of three particles.  Every test prints its own
deviation; DESIGN.md 3.MP has the worst ones measured on an MI355X."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import manyparticle_cases as M  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402

E_REL, F_REL, X_ABS = 1e-10, 1e-9, 1e-12
METHODS = dict(NoCutoff=0, CutoffNonPeriodic=1, CutoffPeriodic=2)
MODES = dict(single=0, central=1)


def assert_close(e, f, e_ref, f_ref, what, e_rel=E_REL):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= e_rel * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


def many_force(name, n, par=None, exclusions=(), method='NoCutoff', cutoff=0.7, mode='single', types=None, filters=None, gvalues=None, group=0):
    case = M.TEXTS[name]
    force = openmm.CustomManyParticleForce(3, case['text'])
    for p in case['names']:
        force.addPerParticleParameter(p)
    for g, value in (case['globals'] if gvalues is None else gvalues).items():
        force.addGlobalParameter(g, value)
    par = np.zeros((n, 0)) if par is None else par
    for k in range(n):
        force.addParticle([float(v) for v in par[k]], 0 if types is None else int(types[k]))
    for a, b in exclusions:
        force.addExclusion(int(a), int(b))
    for r, allowed in enumerate(filters or ()):
        force.setTypeFilter(r, allowed)
    force.setNonbondedMethod(METHODS[method])
    force.setPermutationMode(MODES[mode])
    force.setCutoffDistance(cutoff * unit.nanometers)
    force.setForceGroup(group)
    return force


def twin_force(name, sets, par=None, periodic=False, gvalues=None, group=0):
    """The CustomCompoundBondForce that holds `sets` -- (p1, p2, p3) as the host enumerated them -- as explicit bonds."""
    case = M.compound_case(name, gvalues)
    force = openmm.CustomCompoundBondForce(3, case['text'])
    for p in case['names']:
        force.addPerBondParameter(p)
    for g, value in case['globals'].items():
        force.addGlobalParameter(g, value)
    for members in sets:
        force.addBond([int(m) for m in members], [] if par is None else M.set_parameters(par, members))
    force.setUsesPeriodicBoundaryConditions(periodic)
    force.setForceGroup(group)
    return force


def bare_system(n, box=None, mass=12.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(float(mass))
    if box is not None:
        system.setDefaultPeriodicBoxVectors((float(box[0]), 0, 0), (0, float(box[1]), 0), (0, 0, float(box[2])))
    return system


def context_with(system, positions, integrator=None, properties=None):
    context = openmm.Context(system, integrator or openmm.VerletIntegrator(0.001), None, properties)
    context.setPositions(np.asarray(positions) * unit.nanometers)
    return context


def energy_forces(context, **kw):
    state = context.getState(getEnergy=True, getForces=True, **kw)
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def positions_of(context):
    return context.getState(getPositions=True).getPositions(asNumpy=True)._value


def one_force(n, box, force, positions, properties=None):
    system = bare_system(n, box)
    system.addForce(force)
    context = context_with(system, positions, properties=properties)
    e, f = energy_forces(context)
    context._engine.ctx.check()
    return e, f, context


def stats_of(context):
    return context._engine.many_stats(context._engine.entries[0].force)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def against_the_twin(name, pos, mode, method='NoCutoff', cutoff=None, box=None, exclusions=(), par=None, types=None, filters=None, what=''):
    """The force against the explicit bonds of the host's sets; returns the host's sets and the Context."""
    periodic = method == 'CutoffPeriodic'
    assert cutoff is None or M.margin_ok(pos, cutoff, box if periodic else None)
    sets = M.enumerate_sets(pos, mode == 'central', exclusions, cutoff, box if periodic else None, types, filters)
    force = many_force(name, len(pos), par, exclusions, method, cutoff or 1.0, mode, types, filters)
    e, f, context = one_force(len(pos), box, force, pos)
    stats = stats_of(context)
    assert stats['sets'] == len(sets), (stats, len(sets))
    if not sets:
        assert e == 0.0 and not f.any()
        return sets, context
    e_ref, f_ref, _ = one_force(len(pos), box, twin_force(name, sets, par, periodic), pos)
    assert_close(e, f, e_ref, f_ref, '%s%s (V = %d), n = %d, %s, %s: %d sets, fullest row %d' % (
        what, name, M.N_VARIABLES[name], len(pos), mode, method, len(sets), stats['fullest']))
    return sets, context


# ------------------------------------------------------------------------------------ 1. fails without the feature
def mw_fluid(n, seed=7):
    """An mW-like fluid: one site per molecule, 33.4 per nm^3, on a jittered grid."""
    edge = (n / 33.4) ** (1.0 / 3.0)
    side = int(math.ceil(n ** (1.0 / 3.0)))
    rng = np.random.default_rng(seed)
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)[:n]
    return (grid + 0.5 + rng.uniform(-0.3, 0.3, (n, 3))) * (edge / side), np.full(3, edge)


def test_the_class_runs_in_a_context():
    """On the parent commit: AttributeError, openmm has no CustomManyParticleForce."""
    n = 64
    pos, box = mw_fluid(n)
    rc = M.SW_CUTOFF
    assert M.margin_ok(pos, rc, box)
    force = many_force('stillinger-weber', n, None, (), 'CutoffPeriodic', rc, 'central')
    e, f, context = one_force(n, box, force, pos)
    (entry,) = context._engine.entries
    assert entry.term_expr and len(entry.term_ids) == 1 and entry.bonded_id is None
    assert entry.many['variables'] == [('angle', (1, 0, 2)), ('distance', (0, 1)), ('distance', (0, 2))]
    expected = M.enumerate_sets(pos, True, (), rc, box)
    stats = stats_of(context)
    print('64 mW-like sites, CutoffPeriodic %.5f nm: E = %.12g kJ/mol, max|F| = %.6g, %s (host: %d sets)' % (rc, e, np.abs(f).max(), stats, len(expected)))
    assert math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1e-3
    assert stats['particles'] == n and stats['sets'] == len(expected) > 0 and stats['launches'] >= 2 and stats['capacity'] == 256
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()
    e_ref, f_ref, _ = one_force(n, box, twin_force('stillinger-weber', expected, None, True), pos)
    assert_close(e, f, e_ref, f_ref, 'Stillinger-Weber three-body term, 64 sites')


# ------------------------------------------------------------------------------------ 2. against the 50-digit reference
@pytest.fixture(scope='module')
def bond_cache():
    """The 50-digit bonds already computed, shared by the cases below and never written to but by M.reference."""
    return {}


@pytest.mark.parametrize('method', ('NoCutoff', 'CutoffNonPeriodic', 'CutoffPeriodic'))
@pytest.mark.parametrize('mode', ('single', 'central'))
@pytest.mark.parametrize('n', (3, 4, 6))
@pytest.mark.parametrize('name', ('distance', 'three', 'sixteen'))
def test_small_systems_against_the_50_digit_reference(bond_cache, name, n, mode, method):
    periodic = method == 'CutoffPeriodic'
    central = mode == 'central'
    pos = M.small_layout(n, periodic)
    box = np.full(3, M.SMALL_EDGE)
    cutoff = None if method == 'NoCutoff' else M.SMALL_CUTOFF
    sets = M.enumerate_sets(pos, central, (), cutoff, box if periodic else None)
    e_ref, f_ref, kept, looked = M.reference(name, pos, sets, np.zeros((n, 0)), cutoff, box if periodic else None, central, cache=bond_cache)
    assert looked == len(sets) >= 1 and len(kept) >= M.MIN_KEPT * looked
    e, f, context = one_force(n, box, many_force(name, n, None, (), method, cutoff or 1.0, mode), pos)
    assert stats_of(context)['sets'] == len(sets)
    dropped = [s for s in sets if s not in set(kept)]
    if dropped:         # (the sets the filter drops are taken from the explicit bonds)
        e_d, f_d, _ = one_force(n, box, twin_force(name, dropped, None, periodic), pos)
        e_ref, f_ref = e_ref + e_d, f_ref + f_d
    assert_close(e, f, e_ref, f_ref, '%s (V = %d), n = %d, %s, %s against the 50-digit reference over %d of %d sets' % (
        name, M.N_VARIABLES[name], n, mode, method, len(kept), looked))


@pytest.mark.parametrize('name', ('axilrod-teller', 'with-dihedral'))
def test_named_texts_against_the_50_digit_reference(bond_cache, name):
    n = 6
    pos = M.small_layout(n, False)
    sets = M.enumerate_sets(pos, False)
    e_ref, f_ref, kept, looked = M.reference(name, pos, sets, np.zeros((n, 0)), cache=bond_cache)
    assert looked == 20 and len(kept) >= M.MIN_KEPT * looked
    e, f, _ = one_force(n, None, many_force(name, n), pos)
    dropped = [s for s in sets if s not in set(kept)]
    if dropped:
        e_d, f_d, _ = one_force(n, None, twin_force(name, dropped), pos)
        e_ref, f_ref = e_ref + e_d, f_ref + f_d
    assert_close(e, f, e_ref, f_ref, '%s (V = %d), n = 6, single, NoCutoff against the 50-digit reference' % (name, M.N_VARIABLES[name]))


# ------------------------------------------------------------------------------------ 3. scan, batch and queue boundaries
@pytest.mark.parametrize('mode', ('single', 'central'))
@pytest.mark.parametrize('n', (65, 66))
def test_the_64_column_scan_boundary(n, mode):
    pos = M.positions(n, 1.6, 100 + n, 0.2)
    sets, context = against_the_twin('three', pos, mode)
    assert len(sets) == (3 if mode == 'central' else 1) * n * (n - 1) * (n - 2) // 6 and stats_of(context)['fullest'] == n - 1
    assert stats_of(context)['capacity'] == (n - 1 + 63) // 64 * 64         # 64 and 128


@pytest.mark.parametrize('mode', ('single', 'central'))
def test_neighbour_rows_of_length_1_2_and_12(mode):
    """A pair (no set), a triple (one pair of neighbours) and a cluster of 13 (66 pairs of neighbours: more than one batch)."""
    rc = 0.5
    pos = M.rows_layout(rc)
    assert sorted(len(r) for r in M.neighbours(pos, (), rc)) == [1] * 2 + [2] * 3 + [12] * 13
    sets, _ = against_the_twin('three', pos, mode, 'CutoffNonPeriodic', rc)
    assert len(sets) == (3 if mode == 'central' else 1) * (1 + 286)


@pytest.mark.parametrize('m,removed,target', ((12, 3, 63), (12, 2, 64), (12, 1, 65), (17, 8, 128), (17, 7, 129)))
def test_the_queues_drain_points(m, removed, target):
    """A cluster of m particles around particle 0 under CutoffNonPeriodic, every one inside the cutoff of every other; `removed`
    exclusions between disjoint pairs of the others leave the wavefront of particle 0 with exactly `target` survivors."""
    rc = 0.5
    pos = M.cluster_layout(m, rc, 40 + m)
    excl = [(2 * k + 1, 2 * k + 2) for k in range(removed)]
    sets, _ = against_the_twin('three', pos, 'single', 'CutoffNonPeriodic', rc, None, excl, what='%d survivors on row 0: ' % target)
    assert M.entries_per_owner(sets, m + 1)[0] == target


@pytest.mark.parametrize('mode', ('single', 'central'))
@pytest.mark.parametrize('method', ('CutoffNonPeriodic', 'CutoffPeriodic'))
def test_partial_survival(method, mode):
    """130 particles uniformly in a 2.5 nm box under a 0.9 nm cutoff: a row keeps about a fifth of its columns, and under
    CutoffPeriodic many sets are inside only by the minimum image."""
    edge, rc = 2.5, 0.9
    box = np.full(3, edge)
    pos = M.positions(130, edge, 31, 0.2)
    sets, context = against_the_twin('three', pos, mode, method, rc, box)
    total = (3 if mode == 'central' else 1) * 130 * 129 * 128 // 6
    print('%s, %s: %d of %d sets (%.2f %%)' % (method, mode, len(sets), total, 100.0 * len(sets) / total))
    assert 0 < len(sets) < 0.2 * total
    if method == 'CutoffPeriodic':
        free = set(M.enumerate_sets(pos, mode == 'central', (), rc, None))
        assert len(set(sets) - free) > 100


def test_central_mode_does_not_test_the_satellites_distance():
    """Two satellites on opposite sides of the centre, 1.6 cutoffs apart: a set in central mode, none in single mode."""
    rc = 0.5
    pos = np.array([[1.0, 1.0, 1.0], [1.4, 1.0, 1.02], [0.6, 1.03, 1.0], [1.0, 1.41, 1.0], [1.0, 1.0, 2.5]])
    assert M.distances(pos)[1, 2] > 1.5 * rc
    sets, _ = against_the_twin('three', pos, 'central', 'CutoffNonPeriodic', rc)
    assert (0, 1, 2) in sets and len(sets) == 3          # the centre 0 with its three pairs of satellites; no other centre has two
    sets, _ = against_the_twin('three', pos, 'single', 'CutoffNonPeriodic', rc)
    assert sets == []


# ------------------------------------------------------------------------------------ 4. exclusions
@pytest.mark.parametrize('count', (0, 1, 70))
def test_exclusions_on_one_particle(count):
    rc = 1.2
    pos = M.cluster_layout(75, rc, 55, extra=2)
    excl = [(2, k) for k in range(3, 3 + count)]
    sets, context = against_the_twin('three', pos, 'single', 'CutoffNonPeriodic', rc, None, excl, what='%d exclusions on particle 2: ' % count)
    assert M.entries_per_owner(sets, len(pos))[2] == (75 - count) * (74 - count) // 2 and stats_of(context)['fullest'] == 75


@pytest.mark.parametrize('mode', ('single', 'central'))
def test_an_exclusion_between_two_satellites(mode):
    """(1, 2) excluded: no set holds both, with either as the centre or with another centre; 1 and 2 stay neighbours of the rest."""
    rc = 0.5
    pos = M.cluster_layout(5, rc, 61)
    sets, _ = against_the_twin('three', pos, mode, 'CutoffNonPeriodic', rc, None, [(1, 2)])
    assert sets and not any({1, 2} <= set(s) for s in sets) and any(1 in s for s in sets) and any(2 in s for s in sets)
    assert len(sets) == (3 if mode == 'central' else 1) * (20 - 4)


# ------------------------------------------------------------------------------------ 5. types and filters
@pytest.mark.parametrize('mode', ('single', 'central'))
def test_two_types_with_filters_that_keep_a_b_a(mode):
    rc = 0.5
    pos = M.cluster_layout(11, rc, 71, extra=1)
    types = [7 if k % 3 == 1 else 4 for k in range(len(pos))]           # B = 7, A = 4
    filters = [{4}, {7}, {4}]
    sets, _ = against_the_twin('three', pos, mode, 'CutoffNonPeriodic', rc, None, (), None, types, filters)
    assert sets and all([types[m] for m in s] == [4, 7, 4] for s in sets)
    unfiltered = M.enumerate_sets(pos, mode == 'central', (), rc)
    assert 0 < len(sets) < len(unfiltered)


@pytest.mark.parametrize('mode', ('single', 'central'))
def test_an_asymmetric_text_follows_the_hosts_rule(mode):
    """'sixteen' is not symmetric in p1 p2 p3; with three types and filters that admit several permutations, the device evaluates
    set for set the permutation the host's rule chooses: the same count, and the sum of the explicit bonds in the host's order."""
    rc = 0.5
    pos = M.cluster_layout(12, rc, 83)
    types = [k % 3 for k in range(len(pos))]
    filters = [{0, 1}, {1, 2}, set()]
    sets, context = against_the_twin('sixteen', pos, mode, 'CutoffNonPeriodic', rc, None, (), None, types, filters)
    ascending = [s for s in sets if list(s) == sorted(s)]
    print('%s: %d sets, %d of them in another order than the tuple' % (mode, len(sets), len(sets) - len(ascending)))
    assert 0 < len(ascending) < len(sets) and stats_of(context)['sets'] == len(sets)


# ------------------------------------------------------------------------------------ 6. parameters
def test_parameters_and_their_updates():
    n, rc, name = 40, 0.6, 'parameters'
    pos = M.positions(n, 1.2, 51, 0.2)
    par = M.parameters(name, n, 5)
    types = [k % 2 for k in range(n)]
    assert M.margin_ok(pos, rc)
    sets = M.enumerate_sets(pos, True, (), rc, None, types, [{0}, set(), set()])
    force = many_force(name, n, par, (), 'CutoffNonPeriodic', rc, 'central', types, [{0}, set(), set()])
    e, f, context = one_force(n, None, force, pos)
    e_ref, f_ref, _ = one_force(n, None, twin_force(name, sets, par), pos)
    assert_close(e, f, e_ref, f_ref, 'two per-particle parameters, %d sets' % len(sets))
    # new parameters, new types, a new filter and a new global: the same bits as a Context built with them
    par2 = M.parameters(name, n, 6)
    types2 = [(k // 2) % 3 for k in range(n)]
    for k in range(n):
        force.setParticleParameters(k, [float(v) for v in par2[k]], types2[k])
    force.setTypeFilter(0, [1, 2])
    force.updateParametersInContext(context)
    context.setParameter('scale', 0.7)
    e_new, f_new = energy_forces(context)
    fresh = many_force(name, n, par2, (), 'CutoffNonPeriodic', rc, 'central', types2, [{1, 2}, set(), set()], gvalues=dict(scale=0.7))
    e_fresh, f_fresh, fresh_context = one_force(n, None, fresh, pos)
    print('after updateParametersInContext and setParameter: E = %.15g, fresh Context %.15g' % (e_new, e_fresh))
    assert e_new == e_fresh and np.array_equal(f_new, f_fresh) and e_new != e
    assert stats_of(context)['sets'] == stats_of(fresh_context)['sets'] == len(M.enumerate_sets(pos, True, (), rc, None, types2, [{1, 2}, set(), set()]))


# ------------------------------------------------------------------------------------ 7. determinism
@pytest.mark.parametrize('mode', ('single', 'central'))
def test_same_bits_and_exact_accumulation(mode):
    n = 64
    pos, box = mw_fluid(n)
    force = many_force('stillinger-weber' if mode == 'central' else 'axilrod-teller', n, None, (), 'CutoffPeriodic', M.SW_CUTOFF, mode)
    e0, f0, context = one_force(n, box, force, pos)
    ctx, fid = context._engine.ctx, context._engine.entries[0].term_ids[0]
    e1, f1 = evaluate(ctx, fid, pos)
    e2, f2 = evaluate(ctx, fid, pos)
    _, f3 = evaluate(ctx, fid, pos, energy=False)
    assert e1 == e2 == e0 and np.array_equal(f1, f2) and np.array_equal(f1, f3) and np.array_equal(f1, f0) and f1.any()
    start = np.random.default_rng(5).normal(size=f1.shape) * 100.0
    _, f4 = evaluate(ctx, fid, pos, accumulate=True, start=start, energy=False)
    assert np.array_equal(f4, start + f1)
    ctx.check()


# ------------------------------------------------------------------------------------ 8. capacity
def test_a_row_of_exactly_the_capacity_passes():
    rc = 1.2
    pos = M.cluster_layout(64, rc, 154)
    assert all(len(r) == 64 for r in M.neighbours(pos, (), rc))
    force = many_force('distance', 65, None, (), 'CutoffNonPeriodic', rc, 'single')
    e, f, context = one_force(65, None, force, pos, {'Option.many_capacity': 64})
    stats = stats_of(context)
    assert stats['capacity'] == 64 and stats['fullest'] == 64 and stats['sets'] == 65 * 64 * 63 // 6
    e_wide, f_wide, wide = one_force(65, None, many_force('distance', 65, None, (), 'CutoffNonPeriodic', rc, 'single'), pos)
    assert stats_of(wide)['capacity'] == 256 and e == e_wide and np.array_equal(f, f_wide)


def test_a_row_beyond_the_capacity_is_reported_by_name():
    """A handled flag, not a fault: the row is clamped in the table, amm_check names the capacity and the need, and nothing runs on
    the Context afterwards."""
    rc = 1.2
    pos = M.cluster_layout(65, rc, 155)
    assert all(len(r) == 65 for r in M.neighbours(pos, (), rc))
    system = bare_system(66)
    system.addForce(many_force('distance', 66, None, (), 'CutoffNonPeriodic', rc, 'single'))
    context = context_with(system, pos, properties={'Option.many_capacity': 64})
    with pytest.raises(B.HipError, match=r'neighbour table overflow in many-particle force \d+ \(AMM_FORCE_MANY_PARTICLE\): a particle has 65 '
                                         r'neighbours > capacity 64 \(option many_capacity\)'):
        context.getState(getEnergy=True, getForces=True)          # (getState ends on amm_check)


# ------------------------------------------------------------------------------------ 9. integration
def thermal(n, mass, seed=2026):
    return np.random.default_rng(seed).normal(size=(n, 3)) * math.sqrt(2.494339 / mass)


def test_twenty_verlet_steps_against_the_explicit_bonds():
    n = 12
    pos = M.positions(n, 1.0, 61, 0.25)
    sets = M.enumerate_sets(pos, False)
    assert len(sets) == 220
    xs = []
    for force in (many_force('three', n), twin_force('three', sets)):
        system = bare_system(n)
        system.addForce(force)
        integrator = openmm.VerletIntegrator(0.001)
        context = context_with(system, pos, integrator)
        context.setVelocities(thermal(n, 12.0))
        integrator.step(20)
        xs.append(positions_of(context))
        context._engine.ctx.check()
    worst, moved = np.abs(xs[0] - xs[1]).max(), np.abs(xs[0] - pos).max()
    print('20 Verlet steps against the explicit bonds: max |dx| = %.3e nm, atoms moved up to %.3e nm' % (worst, moved))
    assert moved > 1e-3 and worst <= X_ABS


def water_three_body(data, group=0):
    """The Stillinger-Weber three-body term over the oxygens of a three-site water fixture (angle rows are (H, O, H)): the hydrogens
    are particles of another type that no role takes."""
    oxygens = set(int(a) for a in np.asarray(data['angles'])[:, 1])
    n = len(data['positions'])
    types = [0 if k in oxygens else 1 for k in range(n)]
    return many_force('stillinger-weber', n, None, (), 'CutoffPeriodic', M.SW_CUTOFF, 'central', types, [{0}, {0}, {0}], group=group)


def test_four_respa_steps_fusion_on_and_off(spcfw):
    results = []
    for fuse in (True, False):
        system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
        system = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        system.addForce(water_three_body(spcfw, group=0))
        integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
        context = context_with(system, spcfw['positions'], integrator)
        context.setVelocities(np.random.default_rng(2026).normal(size=spcfw['positions'].shape) *
                              np.sqrt(2.494339 / spcfw['mass'])[:, None])
        context._engine.ctx.set_fuse_inner(fuse)
        assert [(type(e.force).__name__, e.group) for e in context._engine.entries if getattr(e, 'many', None)] == [('CustomManyParticleForce', 0)]
        integrator.step(4)
        results.append((positions_of(context), context._engine.ctx.run_stats()))
        context._engine.ctx.check()
    (x_on, stats_on), (x_off, stats_off) = results
    print('4 RESPA [4, 2, 1] steps: run statistics with fusion %s, without %s' % (stats_on, stats_off))
    assert np.array_equal(x_on, x_off) and stats_on['epilogues'] == 0 and stats_off['epilogues'] == 0
    assert np.abs(x_on - spcfw['positions']).max() > 1e-4


def test_minimisation_lowers_the_energy():
    n = 64
    pos, box = mw_fluid(n)
    system = bare_system(n, box)
    system.addForce(many_force('stillinger-weber', n, None, (), 'CutoffPeriodic', M.SW_CUTOFF, 'central'))
    sim = app.Simulation(app.Topology(n), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(pos * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy(maxIterations=50)
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('minimisation: E %.8g -> %.8g kJ/mol' % (e0, e1))
    assert math.isfinite(e1) and e1 < e0
    sim.context._engine.ctx.check()


def test_langevin_middle_with_a_barostat(spcfw):
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    system.addForce(water_three_body(spcfw, group=5))
    barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 10)
    barostat.setRandomNumberSeed(11)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(3)
    context = context_with(system, spcfw['positions'], integrator)
    context.setVelocitiesToTemperature(300.0, 5)
    integrator.step(50)
    state = context.getState(getEnergy=True, getPositions=True, groups={5})
    e_run = state.getPotentialEnergy()._value
    x = state.getPositions(asNumpy=True)._value
    vectors = state.getPeriodicBoxVectors()
    edges = np.array([vectors[k][k] if not hasattr(vectors[k][k], '_value') else vectors[k][k]._value for k in range(3)], dtype=np.float64)
    stats = context._engine.barostat_stats
    assert stats['attempts'] == 5 and math.isfinite(e_run) and np.isfinite(x).all()
    # a fresh Context at the final box and positions
    fresh = bare_system(len(x), edges)
    fresh.addForce(water_three_body(spcfw, group=5))
    e_fresh, _ = energy_forces(context_with(fresh, x), groups={5})
    print('LangevinMiddle + barostat, 50 steps: %s; box %s -> %s; three-body energy %.12g, fresh Context %.12g (rel %.2e)' % (
        stats, spcfw['box'], edges, e_run, e_fresh, abs(e_run - e_fresh) / abs(e_fresh)))
    assert e_fresh != 0.0 and abs(e_run - e_fresh) <= E_REL * abs(e_fresh)
    context._engine.ctx.check()


def test_free_space_system_runs():
    n = 8
    pos = M.positions(n, 0.9, 71, 0.25)
    system = bare_system(n)
    nb = openmm.NonbondedForce()
    for _ in range(n):
        nb.addParticle(0.0, 0.2, 0.1)
    nb.setNonbondedMethod(nb.NoCutoff)
    system.addForce(nb)
    system.addForce(many_force('three', n, group=1))
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(system, pos, integrator)
    assert context._engine.free_space
    e, f = energy_forces(context, groups={1})
    e_ref, f_ref, _ = one_force(n, None, twin_force('three', M.enumerate_sets(pos, False)), pos)
    assert_close(e, f, e_ref, f_ref, 'free space, NoCutoff, 8 particles')
    integrator.step(10)
    assert np.isfinite(positions_of(context)).all() and np.abs(positions_of(context) - pos).max() > 1e-6
    system.addForce(many_force('three', n, None, (), 'CutoffPeriodic', 0.3))
    with pytest.raises(atomsmm.InputError, match='periodic boundary'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 10. refusals at the C-ABI
def test_abi_refusals_name_the_cause():
    from atomsmm_amd import expr as X
    n = 6
    pos = M.positions(n, 0.8, 3, 0.2) + 0.6
    prog, _ = X.compile_many_particle('distance(p1,p2)', 3, [], [])
    ctx = B.HipContext(n, np.full(3, 2.0))
    nobox = B.HipContext(n, None)
    big = B.HipContext(2049, None)
    try:
        def create(c=ctx, kinds=(B.CVAR_DISTANCE,), slots=((0, 1),), par=None, types=None, n_types=1, table=None, excl=None, rc=0.0, periodic=False,
                   central=False, prog=prog, count=n):
            return c.many_create(prog.code, prog.consts, [], list(kinds), [list(s) for s in slots], np.zeros((0, count)) if par is None else par,
                                 np.zeros(count, dtype=np.int32) if types is None else types, n_types,
                                 np.zeros(n_types ** 3, dtype=np.int32) if table is None else table, excl, rc=rc, periodic=periodic, central=central)
        with pytest.raises(B.HipError, match='amm_many_create: 5 particles, but the context has 6 atoms'):
            create(count=5)
        with pytest.raises(B.HipError, match=r'amm_many_create: 2049 particles under NoCutoff \(limit 2048'):
            create(c=big, count=2049)
        with pytest.raises(B.HipError, match=r'amm_many_create: 17 geometric variables \(limit 16\)'):
            create(kinds=(B.CVAR_DISTANCE,) * 17, slots=((0, 1),) * 17)
        with pytest.raises(B.HipError, match=r'amm_many_create: 3 per-particle parameters \(limit 2'):
            create(par=np.zeros((3, n)))
        with pytest.raises(B.HipError, match=r'amm_many_create: 17 particle types \(limit 16\)'):
            create(n_types=17)
        with pytest.raises(B.HipError, match=r'amm_many_create: particle 2 has the type index 1 \(the force has 1 types\)'):
            create(types=np.array([0, 0, 1, 0, 0, 0], dtype=np.int32))
        with pytest.raises(B.HipError, match=r'amm_many_create: entry 0 of the permutation table is 6'):
            create(table=np.array([6], dtype=np.int32))
        with pytest.raises(B.HipError, match=r'amm_many_create: entry 0 of the permutation table is 2 \(-1: skip; 0 \.\. 1\)'):
            create(table=np.array([2], dtype=np.int32), central=True)
        with pytest.raises(B.HipError, match=r'amm_many_create: exclusion 1 \(particles 6, 0\) is out of range'):
            create(excl=[(0, 1), (6, 0)])
        with pytest.raises(B.HipError, match='amm_many_create: CutoffPeriodic, but the context has no periodic box'):
            create(c=nobox, rc=0.5, periodic=True)
        with pytest.raises(B.HipError, match=r'amm_many_create: the cutoff 1\.10* exceeds half the shortest box edge \(2\.0*\)'):
            create(rc=1.1, periodic=True)
        with pytest.raises(B.HipError, match=r'amm_many_create: variable 0 names slot 3 beyond the set \(3 slots: p1 p2 p3\)'):
            create(slots=((0, 3),))
        with_p = X.compile_many_particle('k1*distance(p1,p2)', 3, ['k'], [])[0]
        with pytest.raises(B.HipError, match=r'amm_many_create: per-term parameter index out of range \(the force has 0\)'):
            create(prog=with_p)
        with pytest.raises(B.HipError, match='amm_set_option: many_capacity is a multiple of 64'):
            ctx.set_option('many_capacity', 100)
        fid = create()
        e, f = evaluate(ctx, fid, pos)
        d = M.distances(pos)
        expected = sum(d[i, j] * (n - 1 - j) for i in range(n) for j in range(i + 1, n))      # distance(p1,p2) of every i < j < k
        assert e == pytest.approx(expected, rel=1e-12) and ctx.many_stats(fid) == dict(particles=6, sets=20, launches=2, fullest=5, capacity=64)
        # the other families refuse the id, naming the type
        for call in (lambda: ctx.bonded_finalize(fid), lambda: ctx.term_expr_set_globals(fid, []), lambda: ctx.compound_set_globals(fid, []),
                     lambda: ctx.hbond_stats(fid), lambda: ctx.pair_set_params(fid, np.zeros(n), np.zeros(n), np.zeros(n))):
            with pytest.raises(B.HipError, match='AMM_FORCE_MANY_PARTICLE'):
                call()
        other, _ = X.compile_compound('distance(p1,p2)', 2, 'p', [], [])
        cid = ctx.compound_create(2, other.code, other.consts, [], [B.CVAR_DISTANCE], [[0, 1]], np.array([[0, 1]], dtype=np.int32), np.zeros((0, 1)))
        with pytest.raises(B.HipError, match=r'amm_many_stats: not the id of a many-particle force \(AMM_FORCE_MANY_PARTICLE\): force %d is a compound-bond force' % cid):
            ctx.many_stats(cid)
        with pytest.raises(B.HipError, match='amm_many_set_globals: the program reads 0 globals, 1 given'):
            ctx.many_set_globals(fid, [1.0])
        with pytest.raises(B.HipError, match='amm_many_set_params: the force has 6 particles of 0 parameters, 6 x 1 given'):
            ctx.many_set_params(fid, np.zeros((1, n)), np.zeros(n, dtype=np.int32), 1, np.zeros(1, dtype=np.int32))
        # a periodic force whose box shrinks under it: refused at the evaluation, by name
        per = create(rc=0.9, periodic=True)
        ctx.set_box(np.full(3, 1.7))
        with pytest.raises(B.HipError, match=r'AMM_FORCE_MANY_PARTICLE\): the cutoff 0\.90* exceeds half the shortest box edge'):
            evaluate(ctx, per, pos)
        ctx.many_release(fid)
        with pytest.raises(B.HipError, match='amm_many_release: not the id of a many-particle force'):
            ctx.many_release(fid)
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, pos)
        ctx.check()
    finally:
        ctx.close()
        nobox.close()
        big.close()
