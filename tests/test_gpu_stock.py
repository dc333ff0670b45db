"""GPU tests (run with -m gpu on an MI355X) of OpenMM's stock integrators: AMM_OP_STOCK (csrc/stock.hip) against the numpy
restatement of its formulas (tests/stock_ref.py) and the exact solutions of the constraint equations (oracle/constraints_oracle.py),
the engine's one-launch step against the same step from the existing ops, and the integrators through the OpenMM-style surface --
Verlet NVE, LangevinMiddle thermalisation, LangevinMiddle + MonteCarloBarostat on rigid water, and a drop-in script.

Bounds: positions 1e-12 nm (the device-against-restatement bound of test_gpu_constraints.py), velocities 1e-12/dt (three of the
four kinds difference positions over dt)."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402
from oracle import constraints_oracle as CO  # noqa: E402  (checker only)
import stock_ref as SR  # noqa: E402

KB = unit.BOLTZMANN_CONSTANT_kB._value
DT, KT, SEED, STEPS = 0.002, KB * 300.0, 20261, 3
FRICTION = {SR.VERLET: 0.0, SR.LANGEVIN_MIDDLE: 5.0, SR.LANGEVIN: 5.0, SR.BROWNIAN: 100.0}     # 1/ps
BOUND_X, BOUND_V = 1e-12, 1e-12 / DT


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


# ------------------------------------------------------------------------------------ 1, 2: the op through the ABI
@functools.lru_cache(maxsize=None)
def synthetic():
    """150 rigid three-site triangles, 40 X-H pairs, 20 four-atom clusters (centre + 3 H), 7 eight-atom chains (7 constraints: the
    generic path at the atom limit) and 63 free atoms with mixed masses, the molecules in random order: 280 work units (more than
    one 256-thread block, a partial last one), every path of the kernel.  Positions on the constraint surface, Gaussian velocities,
    a fixed random force buffer."""
    rng = np.random.default_rng(77)
    kinds = ['tri'] * 150 + ['pair'] * 40 + ['xh3'] * 20 + ['chain'] * 7 + ['free'] * 63
    rng.shuffle(kinds)
    r_oh, r_hh, r_xh, r_cc = 0.09572, 0.15139, 0.109, 0.153
    xs, ms, pairs, dist = [], [], [], []

    def unit_vector():
        a = rng.normal(size=3)
        return a / np.linalg.norm(a)
    for count, kind in enumerate(kinds):
        base, origin = len(xs), rng.uniform(0, 6, 3)
        if kind == 'tri':
            a = unit_vector()
            b = np.cross(a, rng.normal(size=3))
            b /= np.linalg.norm(b)
            half = np.arcsin(0.5 * r_hh / r_oh)
            xs += [origin, origin + r_oh * (np.cos(half) * a + np.sin(half) * b), origin + r_oh * (np.cos(half) * a - np.sin(half) * b)]
            ms += [15.9994, 1.008, 1.008]
            # the constraint orders and orientations a System can come with: createSystem's (H1-O, H2-O, H1-H2), O first, H-H first
            local = [[(1, 0), (2, 0), (1, 2)], [(0, 1), (0, 2), (1, 2)], [(1, 2), (0, 1), (2, 0)]][count % 3]
            d_of = {frozenset((0, 1)): r_oh, frozenset((0, 2)): r_oh, frozenset((1, 2)): r_hh}
            pairs += [(base + i, base + j) for i, j in local]
            dist += [d_of[frozenset(p)] for p in local]
        elif kind == 'pair':
            xs += [origin, origin + r_xh * unit_vector()]
            ms += [12.011, 1.008]
            pairs.append((base + 1, base) if count % 2 else (base, base + 1))
            dist.append(r_xh)
        elif kind == 'xh3':
            xs.append(origin)
            ms.append(14.0067)
            for h in range(3):
                xs.append(origin + r_xh * unit_vector())
                ms.append(1.008 + 0.5 * h)
                pairs.append((base, base + 1 + h))
                dist.append(r_xh)
        elif kind == 'chain':
            xs.append(origin)
            ms.append(12.011)
            for k in range(7):
                xs.append(xs[-1] + r_cc * unit_vector())
                ms.append(12.011 + 1.5 * (k % 3))
                pairs.append((base + k, base + k + 1))
                dist.append(r_cc)
        else:
            xs.append(origin)
            ms.append(float(rng.choice([1.008, 12.011, 15.9994, 35.453])))
    x, mass = np.array(xs), np.array(ms)
    n = len(x)
    assert n == 450 + 80 + 80 + 56 + 63
    v = rng.normal(size=(n, 3)) * np.sqrt(KT / mass)[:, None]
    f = rng.normal(0.0, 300.0, (n, 3))
    return dict(x=x, v=v, f=f, mass=mass, pairs=np.array(pairs, dtype=np.int32), dist=np.array(dist))


@functools.lru_cache(maxsize=None)
def clusters():
    s = synthetic()
    return SR.Clusters(len(s['x']), s['pairs'], s['dist'])


@functools.lru_cache(maxsize=None)
def restated(kind, tol, constrained):
    """The states after steps 1 .. STEPS of the restatement (computed once per case), and the most sweeps a solver call took."""
    s = synthetic()
    x, v, worst, states = s['x'], s['v'], 0, []
    for k in range(1, STEPS + 1):
        x, v, sweeps = SR.step(kind, x, v, s['f'], s['mass'], clusters() if constrained else None, DT, FRICTION[kind], KT, tol, SEED, k)
        worst = max(worst, sweeps)
        states.append((x, v))
    return states, worst


def run_stock(kind, tol, constrained):
    """The op through the ABI, no force kernels: one step, then the other two as a repetition.  Returns the states after step 1 and
    after step STEPS, and the context (to be closed by the caller)."""
    s = synthetic()
    n = len(s['x'])
    ctx = B.HipContext(n, np.array([6.0, 6.0, 6.0]))
    x, v, f = dev(s['x']), dev(s['v']), dev(s['f'])
    ctx.bind_state(x, v, dev(s['mass']))
    ctx.bind_buffer(0, f)
    if constrained:
        ctx.constraints_create(s['pairs'], s['dist'], tol)
    ctx.expr_seed(SEED)
    sid = ctx.stock_define(kind, DT, FRICTION[kind], KT)
    op = B.Op(B.OP_STOCK, sid, 0, 0, 0.0)
    ctx.run_ops([op], 1)
    ctx.check()                         # (the solver's failure flag is clear)
    first = (x.cpu().numpy(), v.cpu().numpy())
    ctx.run_ops([op], STEPS - 1)
    ctx.check()
    return first, (x.cpu().numpy(), v.cpu().numpy()), ctx, (x, v)


def compare(got, want, what):
    dx, dv = np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()
    print('%s: max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e nm/ps (bound %.0e)' % (what, dx, BOUND_X, dv, BOUND_V))
    assert dx < BOUND_X and dv < BOUND_V, what


def counter_advanced_by(ctx, v, mass, steps):
    """One more random op: an Ornstein-Uhlenbeck bath with z = 0 leaves v = sqrt(kT/m) N, N of the next counter of the stream."""
    bid = ctx.bath_define(0.0, KT)
    ctx.run_ops([B.Op(B.OP_BATH, bid, B.SLOT_V, 0, 0.0)], 1)
    ctx.check()
    want = np.sqrt(KT / mass)[:, None] * SR.gaussians(len(mass), SEED, steps + 1)
    assert np.abs(v.cpu().numpy() - want).max() < 1e-13


@pytest.mark.parametrize('tol', [1e-5, 1e-13])
@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE, SR.LANGEVIN, SR.BROWNIAN])
def test_stock_op_against_the_restatement(kind, tol):
    s = synthetic()
    cl = clusters()
    shapes = sorted((len(idx), len(local)) for idx, local, _ in cl.list)
    assert shapes.count((3, 3)) == 150 and shapes.count((2, 1)) == 40 and shapes.count((4, 3)) == 20 and shapes.count((8, 7)) == 7
    assert int((~cl.constrained).sum()) == 63
    states, worst = restated(kind, tol, True)
    print('restatement: at most %d sweeps' % worst)
    assert worst <= 250                  # the reference alone converges well inside the 500 sweeps
    first, last, ctx, (x, v) = run_stock(kind, tol, True)
    compare(first, states[0], 'step 1')
    compare(last, states[-1], 'step %d' % STEPS)
    d = np.linalg.norm(last[0][s['pairs'][:, 0]] - last[0][s['pairs'][:, 1]], axis=1)
    assert np.abs(d / s['dist'] - 1).max() < 1.01 * tol + 5e-14
    if tol == 1e-13 and kind == SR.VERLET:
        # the definition itself: Newton's method on the multipliers of every cluster (test_tight_tolerance_meets_the_exact_solutions)
        x1 = s['x'] + DT * (s['v'] + (DT * s['f']) / s['mass'][:, None])
        for idx, local, dist in cl.list:
            exact = CO.shake_exact(x1[idx], s['x'][idx], s['mass'][idx], local, dist)
            assert np.abs(first[0][idx] - exact).max() < 1e-13
    if kind == SR.LANGEVIN_MIDDLE:
        # the constrained positions are the solver's next reference: a CONSTRAIN_X without SAVE_REF shakes along their bond vectors
        moved = last[0] + np.random.default_rng(5).normal(0, 0.002, last[0].shape)
        x.copy_(dev(moved))
        ctx.run_ops([B.Op(B.OP_CONSTRAIN_X, 0, 0, 0, 0.0)], 1)
        ctx.check()
        want, _ = SR.shake(moved, last[0], s['mass'], cl, tol)
        assert np.abs(x.cpu().numpy() - want).max() < BOUND_X
    counter_advanced_by(ctx, v, s['mass'], STEPS)
    ctx.close()


@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE, SR.LANGEVIN, SR.BROWNIAN])
def test_stock_op_without_constraints(kind):
    """The same inputs and no constraint set: every atom is a free unit."""
    states, _ = restated(kind, 1e-5, False)
    first, last, ctx, (x, v) = run_stock(kind, 1e-5, False)
    compare(first, states[0], 'step 1')
    compare(last, states[-1], 'step %d' % STEPS)
    counter_advanced_by(ctx, v, synthetic()['mass'], STEPS)
    ctx.close()


def test_stock_op_errors():
    s = synthetic()
    ctx = B.HipContext(len(s['x']), np.array([6.0, 6.0, 6.0]))
    x, v = dev(s['x']), dev(s['v'])
    ctx.bind_state(x, v, dev(s['mass']))
    for args, text in [((4, DT, 1.0, KT), 'unknown kind'), ((0, 0.0, 0.0, KT), 'step size must not be 0'), ((-1, DT, 1.0, KT), 'unknown kind'), ((3, DT, 0.0, KT), 'friction > 0'),
                       ((1, DT, -1.0, KT), 'must not be negative'), ((2, DT, 1.0, -KT), 'must not be negative')]:
        with pytest.raises(B.HipError, match=text):
            ctx.stock_define(*args)
    sid = ctx.stock_define(1, DT, 1.0, KT)
    with pytest.raises(B.HipError, match='force buffer not bound'):
        ctx.run_ops([B.Op(B.OP_STOCK, sid, 5, 0, 0.0)], 1)
    f = dev(s['f'])
    ctx.bind_buffer(5, f)
    with pytest.raises(B.HipError, match='unknown stock id'):
        ctx.run_ops([B.Op(B.OP_STOCK, sid + 1, 5, 0, 0.0)], 1)
    w = dev(np.zeros_like(s['x']))
    ctx.bind_buffer(6, w)
    ctx.iso_define(True, KT, 1.0, 6)
    with pytest.raises(B.HipError, match='isokinetic or the regulated mode'):
        ctx.run_ops([B.Op(B.OP_STOCK, sid, 5, 0, 0.0)], 1)
    ctx.iso_define(False)
    ctx.regulated_define(True, 1.0, KT)
    with pytest.raises(B.HipError, match='isokinetic or the regulated mode'):
        ctx.run_ops([B.Op(B.OP_STOCK, sid, 5, 0, 0.0)], 1)
    ctx.regulated_define(False)
    assert np.array_equal(x.cpu().numpy(), s['x']) and np.array_equal(v.cpu().numpy(), s['v'])       # nothing ran
    ctx.run_ops([B.Op(B.OP_STOCK, sid, 5, 0, 0.0)], 1)
    ctx.check()
    ctx.close()


# ------------------------------------------------------------------------------------ 3 .. 7: through the engine
def _rigid_water(spcfw):
    """(as test_gpu_constraints.py builds it)"""
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic', rigidWater=True)
    assert system.getNumConstraints() == 3 * 512
    nb = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    force = atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb)
    force.addTo(system)
    return system


def _flexible_water(spcfw):
    """(as test_gpu_thermostats.py builds it)"""
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    nb = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    force = atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb)
    force.addTo(system)
    return system


def _bond_error(context, system):
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    cons = np.array([(i, j) for i, j, _ in system._constraints])
    d = np.array([d for _, _, d in system._constraints])
    return np.abs(np.linalg.norm(x[cons[:, 0]] - x[cons[:, 1]], axis=1) / d - 1).max()


@pytest.mark.parametrize('name', ['verlet', 'middle'])
def test_native_step_equals_the_op_by_op_step(spcfw, name):
    """q-SPC-FW rigid water (1 536 atoms), three steps from one state with one seed: the one-launch step against the same step from
    KICK, CONSTRAIN_V, MOVE, BATH, COPY, CONSTRAIN_X and EXPR ops."""
    system = _rigid_water(spcfw)
    results = []
    for native in (True, False):
        if name == 'verlet':
            integrator = openmm.VerletIntegrator(2 * unit.femtoseconds)
        else:
            integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 2 * unit.femtoseconds)
        integrator.setRandomNumberSeed(99)
        context = openmm.Context(system, integrator)
        context._engine.set_stock_native(native)
        context.setPositions(spcfw['positions'] * unit.nanometers)
        context.applyConstraints()
        context.setVelocitiesToTemperature(300 * unit.kelvin, 4)
        scheduled = context._engine.ctx.run_stats()['scheduled']
        integrator.step(STEPS)
        per_step = (context._engine.ctx.run_stats()['scheduled'] - scheduled) / STEPS
        state = context.getState(getPositions=True, getVelocities=True)
        results.append((state.getPositions(asNumpy=True)._value, state.getVelocities(asNumpy=True)._value, per_step))
        assert _bond_error(context, system) < 2.1e-5
    (xa, va, la), (xb, vb, lb) = results
    print('%s: ops scheduled per step %.1f native, %.1f op by op; bit-identical: positions %s, velocities %s' %
          (name, la, lb, np.array_equal(xa, xb), np.array_equal(va, vb)))
    assert la == 2 and lb > la                       # the evaluation and ONE op behind it
    assert np.abs(xa - spcfw['positions']).max() > 1e-4
    compare((xa, va), (xb, vb), 'native against op by op')


def test_verlet_conserves_energy_on_rigid_water(spcfw):
    """150 steps of 2 fs: the bounds of test_rigid_water_dynamics_conserves_energy -- bond error < 1e-7 at tolerance 1e-8, |dE| < 0.01 KE.

    The velocities a leapfrog scheme stores are those of t - dt/2, and State.getKineticEnergy() is their sum (OpenMM's half-step
    shift is not made).  The energy that bound is asserted on is therefore the time-centred one, PE(t) + (KE(t - dt/2) + KE(t + dt/2))/2,
    from the State's own numbers one step apart.  PE(t) + KE(t - dt/2), what a single State gives, is off by about (dt/2) sum f.v
    at either end of the run and does not meet the bound, which was made for a velocity-Verlet scheme's on-step velocities: it
    changed by 39.116 kJ/mol against 0.01 KE = 35.112 (MI355X), the time-centred energy by 3.536.  Both are printed."""
    system = _rigid_water(spcfw)
    integrator = openmm.VerletIntegrator(2 * unit.femtoseconds)
    integrator.setConstraintTolerance(1e-8)
    context = openmm.Context(system, integrator)
    context.setPositions(spcfw['positions'] * unit.nanometers)
    context.applyConstraints()
    assert _bond_error(context, system) < 1e-7
    context.setVelocitiesToTemperature(300 * unit.kelvin, 4)

    def energies():
        s = context.getState(getEnergy=True)
        return s.getPotentialEnergy()._value, s.getKineticEnergy()._value
    pe0, ke0 = energies()
    integrator.step(1)
    ke_half = energies()[1]
    integrator.step(149)
    pe1, ke1 = energies()
    error = _bond_error(context, system)
    time = context.getState().getTime()._value
    integrator.step(1)
    ke_next = energies()[1]
    centred = abs((pe1 + 0.5 * (ke1 + ke_next)) - (pe0 + 0.5 * (ke0 + ke_half)))
    print('time-centred: |dE| = %.3f, bound 0.01 KE = %.3f kJ/mol; PE(t) + KE(t - dt/2): |dE| = %.3f' %
          (centred, 0.01 * ke1, abs((pe1 + ke1) - (pe0 + ke0))))
    assert error < 1e-7
    assert centred < 0.01 * ke1
    assert abs(pe1 - pe0) > 1.0                          # something did move
    assert time == pytest.approx(0.3, rel=1e-12)


def test_langevin_middle_equilibrates(spcfw):
    """A cold start reaches the bath temperature: the bounds of test_langevin_middle_scheme_equilibrates, on its system."""
    c = spcfw
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 20 / unit.picoseconds, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(1234)
    context = openmm.Context(_flexible_water(c), integrator)
    context.setPositions(c['positions'] * unit.nanometers)
    context.setVelocitiesToTemperature(30 * unit.kelvin, 1)
    temps = []
    for _ in range(12):
        integrator.step(50)
        ke = context.getState(getEnergy=True).getKineticEnergy()._value
        temps.append(2 * ke / (3 * len(c['mass']) * KB))
    print('block temperatures:', ' '.join('%.1f' % t for t in temps))
    assert temps[0] > 60 and abs(np.mean(temps[-4:]) - 300) < 25, temps
    assert np.isfinite(context.getState(getEnergy=True).getPotentialEnergy()._value)


BAROSTAT_SEED = 1         # (chosen so that an attempt is accepted; the test prints every decision)


def test_langevin_middle_with_barostat_on_rigid_water(spcfw):
    """The equilibration protocol: NPT with LangevinMiddleIntegrator(300 K, 1/ps, 2 fs) and MonteCarloBarostat on rigid water."""
    system = _rigid_water(spcfw)
    barostat = openmm.MonteCarloBarostat(1 * unit.bar, 300 * unit.kelvin, 10)
    barostat.setRandomNumberSeed(BAROSTAT_SEED)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 2 * unit.femtoseconds)
    integrator.setConstraintTolerance(1e-8)
    integrator.setRandomNumberSeed(7)
    context = openmm.Context(system, integrator)
    context.setPositions(spcfw['positions'] * unit.nanometers)
    context.applyConstraints()
    context.setVelocitiesToTemperature(300 * unit.kelvin, 4)
    integrator.step(100)
    eng = context._engine
    print('attempts:', ' '.join('%s(w=%.3f)' % ('accepted' if e[0] else 'rejected', e[1]) for e in eng.barostat_log))
    assert eng.barostat_stats['attempts'] == 10 and eng.barostat_stats['accepted'] >= 1
    assert np.abs(eng.box - spcfw['box']).max() > 1e-6
    assert _bond_error(context, system) < 1e-7
    state = context.getState(getEnergy=True)
    assert np.isfinite(state.getPotentialEnergy()._value) and np.isfinite(state.getKineticEnergy()._value)


def test_drop_in_script():
    """A plain OpenMM script: createSystem(rigidWater=True), LangevinMiddleIntegrator, minimizeEnergy, step."""
    from simtk import openmm as mm
    from simtk import unit as u
    from simtk.openmm import app
    case = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data', 'q-SPC-FW')
    pdb = app.PDBFile(case + '.pdb')
    forcefield = app.ForceField(case + '.xml')
    system = forcefield.createSystem(pdb.topology, nonbondedMethod=app.PME, nonbondedCutoff=1 * u.nanometer, rigidWater=True)
    assert system.getNumConstraints() == 3 * 512
    integrator = mm.LangevinMiddleIntegrator(300 * u.kelvin, 1 / u.picosecond, 2 * u.femtoseconds)
    simulation = app.Simulation(pdb.topology, system, integrator)
    simulation.context.setPositions(pdb.positions)
    simulation.minimizeEnergy(maxIterations=20)
    simulation.context.setVelocitiesToTemperature(300 * u.kelvin, 3)
    e0 = simulation.context.getState(getEnergy=True).getPotentialEnergy()
    simulation.step(20)
    state = simulation.context.getState(getEnergy=True, getPositions=True)
    assert np.isfinite(state.getPotentialEnergy() / state.getPotentialEnergy().unit)
    assert state.getPotentialEnergy() != e0
    assert _bond_error(simulation.context, system) < 2.1e-5
    assert state.getTime() / u.picosecond == pytest.approx(0.04, rel=1e-12)
