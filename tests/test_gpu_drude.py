"""GPU tests (run with -m gpu on an MI355X) of DrudeForce (csrc/drude.hip, AMM_FORCE_DRUDE) and of the DrudeLangevinIntegrator step
(AMM_OP_DRUDE_STEP) against the numpy restatement of their formulas (tests/drude_ref.py) on the cases of tests/drude_cases.py.

Bounds: energy 1e-10 relative, forces 1e-9 of the largest force component (the project's bar for an fp64 force against its
restatement); a device step against the restated step applied to the device's previous state: positions 1e-12 nm, velocities 1e-12/dt
(the bounds of tests/test_gpu_stock.py; the restatement sweeps SHAKE as the kernel does, so they hold at any constraint tolerance, and
the constrained distances themselves are held to 1.01 tol + 5e-14 as there)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import drude_cases as DC  # noqa: E402
import drude_ref as DR  # noqa: E402
import stock_ref as SR  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.testing import swm4_box, swm4_system  # noqa: E402

KB = unit.BOLTZMANN_CONSTANT_kB._value
E_REL, F_REL = 1e-10, 1e-9
BOUND_X = 1e-12


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(context, groups=-1):
    state = context.getState(getEnergy=True, getForces=True, groups=groups)
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def compare_force(name, got, want):
    (e, f), (e0, f0) = got, want
    fmax = np.abs(f0).max()
    de, df = abs(e - e0) / abs(e0), np.abs(f - f0).max() / fmax
    print('%s: |dE|/|E| = %.2e (bound %.0e), max|dF|/max|F| = %.2e (bound %.0e), E = %.6g, max|F| = %.4g' % (name, de, E_REL, df, F_REL, e0, fmax))
    assert de < E_REL and df < F_REL, name


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's answer for a small case, computed once."""
    case = DC.small_cases()[name]
    return DR.energy_forces(case['x'], case['rows'], case['pairs'], case['box'] if case['periodic'] else None)


# ------------------------------------------------------------------------------------ the force
@pytest.mark.parametrize('name', sorted(DC.small_cases()))
def test_energy_and_forces_against_the_restatement(name):
    case = DC.small_cases()[name]
    system, force = DC.system_of(case)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(case['x'])
    first = evaluate(context)
    compare_force(name, first, reference(name))
    second = evaluate(context)
    assert first[0] == second[0] and np.array_equal(first[1], second[1])       # the same positions give the same bits
    forces_only = context.getState(getForces=True).getForces(asNumpy=True)._value
    assert np.array_equal(forces_only, first[1])                                # ... with and without the energy


@functools.lru_cache(maxsize=None)
def swm4():
    case = swm4_box(3)
    rows = [tuple(r) for r in case['drude']]
    return case, rows, DR.energy_forces(case['positions'], rows, [], case['box'])


def swm4_context(integrator=None, barostat=False):
    case, rows, _ = swm4()
    system, force = swm4_system(case, nonbondedMethod='PME')
    if barostat:
        baro = openmm.MonteCarloBarostat(1 * unit.bar, 300 * unit.kelvin, 1)
        baro.setRandomNumberSeed(3)
        system.addForce(baro)
    context = openmm.Context(system, integrator or openmm.VerletIntegrator(0.001))
    context.setPositions(case['positions'])
    return context, system, force


def test_swm4_under_pme_in_its_own_group():
    """(f): 27 polarizable waters under PME; the DrudeForce is group 1, the NonbondedForce group 0."""
    case, rows, want = swm4()
    context, system, force = swm4_context()
    got = evaluate(context, groups={1})
    compare_force('f', got, want)
    again = evaluate(context, groups={1})
    assert got[0] == again[0] and np.array_equal(got[1], again[1])
    e_all, f_all = evaluate(context)
    e_nb, f_nb = evaluate(context, groups={0})
    assert np.isfinite(e_all) and e_all == pytest.approx(e_nb + got[0], rel=1e-12)
    assert np.abs(f_all - (f_nb + got[1])).max() < 1e-9 * np.abs(f_all).max()
    assert np.abs(got[1][4::5]).max() == 0.0 and np.abs(got[1][2::5]).max() == 0.0       # nothing on M or on the hydrogens


def test_update_parameters_in_context():
    """New alpha, q, thole and aniso values are followed; the counts and the particles stay."""
    case = dict(DC.case_d(65))
    system, force = DC.system_of(case)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(case['x'])
    before = evaluate(context)
    rows = [list(r) for r in case['rows']]
    for k, row in enumerate(rows):
        row[5] *= 1.0 + 0.01 * (k % 5)
        row[6] *= 1.1 - 0.02 * (k % 3)
        row[7] = 0.75 + 0.01 * (k % 13)
        row[8] = 1.1 - 0.01 * (k % 9)
        force.setParticleParameters(k, *row)
    pairs = [(a, b, 3.9 - t) for a, b, t in case['pairs']]
    for k, pair in enumerate(pairs):
        force.setScreenedPairParameters(k, *pair)
    force.updateParametersInContext(context)
    after = evaluate(context)
    want = DR.energy_forces(case['x'], [tuple(r) for r in rows], pairs, None)
    compare_force('d65 with new parameters', after, want)
    assert abs(after[0] - before[0]) > 1e-3 * abs(before[0])
    rows[0][1], rows[0][0] = rows[0][0], rows[0][1]
    force.setParticleParameters(0, *rows[0])
    with pytest.raises(openmm.OpenMMException, match='a particle of a Drude particle has changed'):
        force.updateParametersInContext(context)


def test_minimize_energy_on_swm4():
    context, system, force = swm4_context()
    e0 = evaluate(context)[0]
    openmm.LocalEnergyMinimizer.minimize(context, tolerance=10.0, maxIterations=60)
    e1 = evaluate(context)[0]
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    d = np.linalg.norm(x[1::5] - x[0::5], axis=1)
    print('minimizeEnergy: %.3f -> %.3f kJ/mol, |d| from %.2e to %.2e nm' % (e0, e1, d.min(), d.max()))
    assert e1 < e0 and d.min() > 0.0 and d.max() < 0.05


def test_barostat_attempt_keeps_the_drude_particles_on_their_oxygens():
    case, rows, _ = swm4()
    context, system, force = swm4_context(barostat=True)
    x0 = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    engine = context._engine
    for _ in range(4):
        engine._barostat_attempt()
    x1 = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    assert engine.barostat_stats['attempts'] == 4
    moved = np.abs(x1 - x0).max()
    print('barostat: %d of 4 accepted, largest displacement %.3e nm' % (engine.barostat_stats['accepted'], moved))
    assert np.abs((x1[1::5] - x1[0::5]) - (x0[1::5] - x0[0::5])).max() < 1e-12
    assert np.abs((x1[2::5] - x1[0::5]) - (x0[2::5] - x0[0::5])).max() < 1e-12
    assert engine.barostat_stats['accepted'] == 0 or moved > 1e-6


# ------------------------------------------------------------------------------------ the step
DT, T, TD, G, GD, SEED = 0.001, 300.0, 1.0, 5.0, 20.0, 4711


def drude_integrator(dt=DT, friction=G, drude_friction=GD, wall=0.0, seed=SEED):
    integ = openmm.DrudeLangevinIntegrator(T * unit.kelvin, friction / unit.picosecond, TD * unit.kelvin, drude_friction / unit.picosecond,
                                           dt * unit.picoseconds)
    integ.setRandomNumberSeed(seed)
    integ.setMaxDrudeDistance(wall)
    return integ


def state_of(context):
    s = context.getState(getPositions=True, getVelocities=True, getForces=True)
    return s.getPositions(asNumpy=True)._value, s.getVelocities(asNumpy=True)._value, s.getForces(asNumpy=True)._value


def follow(context, integ, mass, pairs, clusters, steps, wall=0.0, tol=1e-5):
    """`steps` device steps, each against the restated step applied to the device's previous state.  Returns the worst deviations."""
    n = len(mass)
    massive = mass > 0
    worst_x = worst_v = 0.0
    for k in range(1, steps + 1):
        x, v, f = state_of(context)
        integ.step(1)
        xn, vn, _ = state_of(context)
        wx, wv, flagged, sweeps = DR.step(x, v, f, mass, pairs, clusters, DT, G, KB * T, GD, KB * TD, wall, tol, SR.gaussians(n, SEED, k))
        assert not flagged and sweeps <= 250
        worst_x = max(worst_x, np.abs(xn - wx)[massive].max())
        worst_v = max(worst_v, np.abs(vn - wv)[massive].max())
        assert np.abs(xn - x)[massive].max() > 1e-6                      # something moved
        assert np.array_equal(vn[~massive], v[~massive])
    print('%d steps: max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e nm/ps (bound %.0e)' % (steps, worst_x, BOUND_X, worst_v, BOUND_X / DT))
    assert worst_x < BOUND_X and worst_v < BOUND_X / DT


def test_ten_steps_unconstrained_against_the_restatement():
    """(d), 129 Drude particles: 258 work units, more than one block; every atom is a lone pair's half."""
    case = DC.case_d(129)
    system, force = DC.system_of(case)
    integ = drude_integrator()
    context = openmm.Context(system, integ)
    context.setPositions(case['x'])
    context.setVelocitiesToTemperature(300 * unit.kelvin, 5)
    pairs = [(r[0], r[1]) for r in case['rows']]
    follow(context, integ, case['mass'], pairs, None, 10)
    t_sys, t_drude = integ.computeSystemTemperature()._value, integ.computeDrudeTemperature()._value
    v = context.getState(getVelocities=True).getVelocities(asNumpy=True)._value
    want = DR.temperatures(v, case['mass'], pairs)
    assert t_sys == pytest.approx(want[0], rel=1e-12) and t_drude == pytest.approx(want[1], rel=1e-12)


def test_ten_steps_on_rigid_swm4_against_the_restatement():
    """(f): the rigid triangle with the Drude particle on its oxygen, M placed afterwards."""
    case, rows, _ = swm4()
    integ = drude_integrator()
    context, system, force = swm4_context(integ)
    context.setVelocities(case['velocities'])
    cons = system._constraints
    clusters = SR.Clusters(len(case['mass']), np.array([(c[0], c[1]) for c in cons]), np.array([c[2] for c in cons]))
    follow(context, integ, case['mass'], [(r[0], r[1]) for r in rows], clusters, 10)
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    d = np.array([np.linalg.norm(x[c[0]] - x[c[1]]) / c[2] - 1 for c in cons])
    assert np.abs(d).max() < 1.01 * 1e-5 + 5e-14
    w = case['sites'][0][5]
    assert np.abs(x[4::5] - ((1 - 2 * w) * x[0::5] + w * x[2::5] + w * x[3::5])).max() < BOUND_X


def test_an_empty_drude_force_gives_langevin_bits():
    """No Drude particles: every atom is an ordinary one, and the arithmetic is AMM_STOCK_LANGEVIN's operation by operation."""
    case, rows, _ = swm4()
    results = []
    for drude in (False, True):
        system, _ = swm4_system(case, nonbondedMethod='PME', drude=False)
        bonds = openmm.HarmonicBondForce()
        for r in rows:
            bonds.addBond(r[0], r[1], 0.0, 4.0e5)
        system.addForce(bonds)
        if drude:
            system.addForce(openmm.DrudeForce())
            integ = drude_integrator(seed=99)
        else:
            integ = openmm.LangevinIntegrator(T * unit.kelvin, G / unit.picosecond, DT * unit.picoseconds)
            integ.setRandomNumberSeed(99)
        context = openmm.Context(system, integ)
        context.setPositions(case['positions'])
        context.setVelocities(case['velocities'])
        integ.step(5)
        s = context.getState(getPositions=True, getVelocities=True)
        results.append((s.getPositions(asNumpy=True)._value, s.getVelocities(asNumpy=True)._value))
    (xa, va), (xb, vb) = results
    assert np.abs(xa - case['positions']).max() > 1e-5
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)


def test_energy_is_conserved_without_friction():
    """gamma = gamma_D = 0 on (d): 200 steps of 0.5 fs.  The allowed drift -- the largest |E(t) - E(0)| over the run, sampled every 10
    steps -- is twice what VerletIntegrator shows on the same System, step count and step size, measured here."""
    case = DC.case_d(65)
    drift = {}
    for name in ('verlet', 'drude'):
        system, force = DC.system_of(case)
        if name == 'verlet':
            integ = openmm.VerletIntegrator(0.0005)
        else:
            integ = openmm.DrudeLangevinIntegrator(T * unit.kelvin, 0.0, TD * unit.kelvin, 0.0, 0.0005)
            integ.setRandomNumberSeed(1)
        context = openmm.Context(system, integ)
        context.setPositions(case['x'])
        context.setVelocitiesToTemperature(300 * unit.kelvin, 9)

        def total():
            s = context.getState(getEnergy=True)
            return s.getPotentialEnergy()._value + s.getKineticEnergy()._value
        e0 = total()
        worst = 0.0
        for _ in range(20):
            integ.step(10)
            worst = max(worst, abs(total() - e0))
        drift[name] = worst
    print('largest |E(t) - E(0)| over 200 steps of 0.5 fs: Verlet %.4e, DrudeLangevin without friction %.4e kJ/mol' % (drift['verlet'], drift['drude']))
    assert drift['verlet'] > 0 and drift['drude'] <= 2 * drift['verlet']


# ------------------------------------------------------------------------------------ the op through the ABI
def run_op(x, v, f, mass, pairs, steps, wall, friction=G, drude_friction=GD, seed=SEED, each=None, constraints=None, tol=1e-5):
    """The op through the ABI, no force kernels: `steps` steps on a fixed force buffer."""
    n = len(x)
    ctx = B.HipContext(n, np.array([50.0, 50.0, 50.0]))
    dx, dv, df = dev(x), dev(v), dev(f)
    ctx.bind_state(dx, dv, dev(mass))
    ctx.bind_buffer(0, df)
    if constraints is not None:
        ctx.constraints_create(constraints[0], constraints[1], tol)
    ctx.expr_seed(seed)
    sid = ctx.drude_step_define(pairs, DT, friction, KB * T, drude_friction, KB * TD, wall)
    op = B.Op(B.OP_DRUDE_STEP, sid, 0, 0, 0.0)
    for k in range(steps):
        ctx.run_ops([op], 1)
        if each is not None:
            each(dv.cpu().numpy())
    ctx.check()
    out = dx.cpu().numpy(), dv.cpu().numpy()
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def mixed_clusters():
    """Every shape of the step kernel with Drude particles on it, the molecules in random order: 70 X-H pairs with a Drude particle on
    X (the two-atom instantiation), 40 rigid triangles with one on the first vertex and 10 with one on every vertex, 20 four-atom
    clusters (centre + 3 H) with one on the centre and 6 eight-atom chains with one on every other atom (the generic sweep), 30 lone
    pairs, 20 lone atoms and 5 massless ones: more than 256 units, several blocks."""
    rng = np.random.default_rng(2027)
    kinds = ['xh'] * 70 + ['tri1'] * 40 + ['tri3'] * 10 + ['xh3'] * 20 + ['chain'] * 6 + ['pair'] * 30 + ['free'] * 20 + ['massless'] * 5
    rng.shuffle(kinds)
    r_oh, r_hh, r_xh, r_cc = 0.09572, 0.15139, 0.109, 0.153
    xs, ms, cons, dist, pairs = [], [], [], [], []

    def unit_vector():
        a = rng.normal(size=3)
        return a / np.linalg.norm(a)

    def drude_on(parent):
        xs.append(xs[parent] + rng.normal(scale=0.006, size=3))
        ms.append(0.4)
        pairs.append((len(xs) - 1, parent))
    for kind in kinds:
        base, origin = len(xs), rng.uniform(0, 40, 3)
        if kind == 'xh':
            xs += [origin, origin + r_xh * unit_vector()]
            ms += [12.011, 1.008]
            cons.append((base, base + 1))
            dist.append(r_xh)
            drude_on(base)
        elif kind in ('tri1', 'tri3'):
            a = unit_vector()
            b = np.cross(a, rng.normal(size=3))
            b /= np.linalg.norm(b)
            half = np.arcsin(0.5 * r_hh / r_oh)
            xs += [origin, origin + r_oh * (np.cos(half) * a + np.sin(half) * b), origin + r_oh * (np.cos(half) * a - np.sin(half) * b)]
            ms += [15.5994, 1.008, 1.008] if kind == 'tri1' else [15.5994, 12.0, 14.0]
            cons += [(base, base + 1), (base, base + 2), (base + 1, base + 2)]
            dist += [r_oh, r_oh, r_hh]
            for k in range(1 if kind == 'tri1' else 3):
                drude_on(base + k)
        elif kind == 'xh3':
            xs.append(origin)
            ms.append(14.0067)
            for h in range(3):
                xs.append(origin + r_xh * unit_vector())
                ms.append(1.008 + 0.5 * h)
                cons.append((base, base + 1 + h))
                dist.append(r_xh)
            drude_on(base)
        elif kind == 'chain':
            xs.append(origin)
            ms.append(12.011)
            for k in range(7):
                xs.append(xs[-1] + r_cc * unit_vector())
                ms.append(12.011 + 1.5 * (k % 3))
                cons.append((base + k, base + k + 1))
                dist.append(r_cc)
            for k in range(0, 8, 2):
                drude_on(base + k)
        elif kind == 'pair':
            xs.append(origin)
            ms.append(15.999)
            drude_on(base)
        else:
            xs.append(origin)
            ms.append(0.0 if kind == 'massless' else 35.453)
    x, mass = np.array(xs), np.array(ms)
    v = rng.normal(size=x.shape) * np.sqrt(KB * T / np.where(mass > 0, mass, 1.0))[:, None]
    v[mass == 0] = 0.0
    f = rng.normal(0.0, 300.0, x.shape)
    return dict(x=x, v=v, f=f, mass=mass, cons=np.array(cons, dtype=np.int32), dist=np.array(dist), pairs=np.array(pairs, dtype=np.int32))


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
def test_every_cluster_shape_against_the_restatement(tol):
    """Three steps of the op on a fixed force buffer; the hard wall is on and far enough to stay out of the way of most pairs."""
    s = mixed_clusters()
    n, wall = len(s['x']), 0.015
    clusters = SR.Clusters(n, s['cons'], s['dist'])
    shapes = sorted((len(idx), len(local)) for idx, local, _ in clusters.list)
    assert shapes.count((2, 1)) == 70 and shapes.count((3, 3)) == 50 and shapes.count((4, 3)) == 20 and shapes.count((8, 7)) == 6
    x, v, reflected = s['x'], s['v'], 0
    for k in range(1, 4):
        free = DR.step(x, v, s['f'], s['mass'], s['pairs'], clusters, DT, G, KB * T, GD, KB * TD, 0.0, tol, SR.gaussians(n, SEED, k))
        x, v, flagged, sweeps = DR.step(x, v, s['f'], s['mass'], s['pairs'], clusters, DT, G, KB * T, GD, KB * TD, wall, tol, SR.gaussians(n, SEED, k))
        reflected += int((np.abs(free[0] - x).max(axis=1) > 0).sum())
        assert not flagged and sweeps <= 250
    got_x, got_v = run_op(s['x'], s['v'], s['f'], s['mass'], s['pairs'], 3, wall, constraints=(s['cons'], s['dist']), tol=tol)
    dx, dv = np.abs(got_x - x).max(), np.abs(got_v - v).max()
    print('tolerance %g: max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e nm/ps (bound %.0e); the wall moved %d atoms' % (tol, dx, BOUND_X, dv, BOUND_X / DT, reflected))
    assert dx < BOUND_X and dv < BOUND_X / DT
    assert np.array_equal(got_x[s['mass'] == 0], s['x'][s['mass'] == 0])
    assert np.abs(got_x - s['x']).max() > 1e-4


def test_hard_wall_against_the_restatement():
    """70 pairs around the wall R = 0.02 nm -- inside, in the reflection zone moving apart and moving together -- and three with a
    massless parent; pair 0 starts just inside R with an outward relative velocity."""
    rng = np.random.default_rng(12)
    n_pairs, R = 70, 0.02
    mass = np.tile([15.6, 0.4], n_pairs)
    mass[[20, 40, 60]] = 0.0                                # massless parents of pairs 10, 20, 30
    pairs = np.array([(2 * k + 1, 2 * k) for k in range(n_pairs)])
    x = np.empty((2 * n_pairs, 3))
    x[0::2] = rng.uniform(0, 5, (n_pairs, 3))
    u = rng.normal(size=(n_pairs, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x[1::2] = x[0::2] + u * (R * rng.uniform(0.8, 1.15, n_pairs))[:, None]
    v = rng.normal(size=(2 * n_pairs, 3)) * 0.3
    v[1::2] += u * rng.normal(0.0, 4.0, n_pairs)[:, None]
    v[mass == 0] = 0.0
    x[1] = x[0] + u[0] * 0.0199
    v[0], v[1] = [0.1, -0.2, 0.05], np.array([0.1, -0.2, 0.05]) + 3.0 * u[0]
    f = rng.normal(0.0, 100.0, x.shape)
    N = SR.gaussians(2 * n_pairs, SEED, 1)
    want_x, want_v, flagged, _ = DR.step(x, v, f, mass, pairs, None, DT, G, KB * T, GD, KB * TD, R, 1e-5, N)
    free_x, free_v, _, _ = DR.step(x, v, f, mass, pairs, None, DT, G, KB * T, GD, KB * TD, 0.0, 1e-5, N)
    assert not flagged
    hit = np.linalg.norm(free_x[1::2] - free_x[0::2], axis=1) > R
    assert hit[0] and 10 < hit.sum() < 60 and hit[[10, 20, 30]].any()
    got_x, got_v = run_op(x, v, f, mass, pairs, 1, R)
    dx, dv = np.abs(got_x - want_x).max(), np.abs(got_v - want_v).max()
    print('hard wall: %d of %d pairs reflected; max|dx| = %.2e nm, max|dv| = %.2e nm/ps' % (hit.sum(), n_pairs, dx, dv))
    assert dx < BOUND_X and dv < BOUND_X / DT
    assert np.linalg.norm(got_x[1] - got_x[0]) <= R * (1 + 1e-12)
    # the wall changes no pair's momentum: what the thermostat left (the run without a wall) is what the run with it has
    p_wall = mass[1::2, None] * got_v[1::2] + mass[0::2, None] * got_v[0::2]
    p_free = mass[1::2, None] * free_v[1::2] + mass[0::2, None] * free_v[0::2]
    massive_parent = mass[0::2] > 0
    assert np.abs(p_wall - p_free)[massive_parent].max() < 1e-9
    assert np.array_equal(got_x[mass == 0], x[mass == 0])


def test_a_pair_beyond_twice_the_wall_raises_and_leaves_no_flag_behind():
    """(The step is 0.1 fs: at 1 fs the spring, (omega dt)^2 = 1.05, would throw the particle from 0.05 nm back inside the wall.)"""
    case = DC.case_a()
    x = case['x'].copy()
    x[1] = x[0] + [0.05, 0.0, 0.0]
    system, force = DC.system_of(case)
    integ = drude_integrator(dt=0.0001, wall=0.02)
    context = openmm.Context(system, integ)
    context.setPositions(x)
    with pytest.raises(openmm.OpenMMException, match='Drude particle moved too far beyond hard wall constraint'):
        integ.step(1)
    system, force = DC.system_of(case)
    integ = drude_integrator(wall=0.02)
    fresh = openmm.Context(system, integ)
    fresh.setPositions(case['x'])
    fresh._engine.ctx.check()
    integ.step(2)
    fresh._engine.ctx.check()


def test_both_temperatures_on_force_free_pairs():
    """512 force-free pairs, 2 000 steps from the stationary distribution: the time averages of both temperatures within 5 standard
    errors, T sqrt(2 tau_int/(n_dof n_steps)) with tau_int = (1 + a^2)/(1 - a^2) (derived in tests/test_drude_host.py)."""
    n_pairs, n_steps, g, gd = 512, 2000, 20.0, 80.0
    rng = np.random.default_rng(8)
    m1, m2 = 0.4, 15.6
    M, mu = m1 + m2, m1 * m2 / (m1 + m2)
    mass = np.tile([m2, m1], n_pairs)
    pairs = np.array([(2 * k + 1, 2 * k) for k in range(n_pairs)])
    vcm = rng.normal(size=(n_pairs, 3)) * math.sqrt(KB * T / M)
    vrel = rng.normal(size=(n_pairs, 3)) * math.sqrt(KB * TD / mu)
    v = np.empty((2 * n_pairs, 3))
    v[1::2] = vcm + vrel * m2 / M
    v[0::2] = vcm - vrel * m1 / M
    x = np.repeat(rng.uniform(0, 40, (n_pairs, 3)), 2, axis=0)
    sums = [0.0, 0.0]

    def each(vk):
        ts, td = DR.temperatures(vk, mass, pairs)
        sums[0] += ts / n_steps
        sums[1] += td / n_steps
    run_op(x, v, np.zeros_like(x), mass, pairs, n_steps, 0.0, friction=g, drude_friction=gd, seed=31, each=each)

    def standard_error(temp, a):
        return temp * math.sqrt(2 * (1 + a * a) / (1 - a * a) / (3 * n_pairs * n_steps))
    se, sed = standard_error(T, math.exp(-g * DT)), standard_error(TD, math.exp(-gd * DT))
    print('system %.3f K (300 +- %.3f), Drude %.5f K (1 +- %.5f)' % (sums[0], se, sums[1], sed))
    assert abs(sums[0] - T) < 5 * se and abs(sums[1] - TD) < 5 * sed
