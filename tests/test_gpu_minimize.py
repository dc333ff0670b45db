"""GPU tests of the energy minimiser: the vector kernels of csrc/minimize.hip through the C-ABI against exact sums and the numpy
restatement (tests/minimize_ref.py), and LocalEnergyMinimizer / Simulation.minimizeEnergy end to end against the CPU oracle."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays, tip3p_box  # noqa: E402
from atomsmm_amd.utils import InputError  # noqa: E402
from minimize_ref import GramLBFGS, minimize as minimize_ref  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from oracle.respa_cpu import RespaCPU  # noqa: E402


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


# ---------------------------------------------------------------------------------------------- 1. vector kernels

def _drive(ctx, n, m, xs, gs, mass=None, max_step=0.1):
    """begin + advances over the given points; returns everything the object shows."""
    scal = torch.zeros(8, dtype=torch.float64, device='cuda')
    d_mass = None if mass is None else dev(mass)
    mid = ctx.min_create(scal, mass=d_mass, memory=m, max_step=max_step, force_input=False)
    ctx.min_begin(mid, dev(xs[0]), dev(gs[0]))
    blocks = [ctx.min_scalars(mid)]
    for x, g in zip(xs[1:], gs[1:]):
        ctx.min_advance(mid, dev(x), dev(g))
        blocks.append(ctx.min_scalars(mid))
    out = dict(blocks=blocks, gram=ctx.min_read(mid, 'gram', m), delta=ctx.min_read(mid, 'delta', m),
               direction=ctx.min_read(mid, 'direction', m), stats=ctx.min_stats(mid))
    x_out = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
    ctx.min_trial(mid, 1.0, x_out)
    out['trial'] = x_out.cpu().numpy()
    out['after_trial'] = ctx.min_scalars(mid)
    ctx.min_release(mid)
    return out


@pytest.mark.parametrize('n', [1, 341, 21846])
def test_vector_kernels_through_the_abi(n):
    """One lane, a ragged tail (3n = 1023) and several blocks; m = 3, five random points, so the ring wraps once.
    Gram entries against math.fsum of the products within 1e-13 sum|a_i b_i| (log2(3n) <= 17 rounding steps of 1.1e-16), max|g|
    exactly, two runs bit for bit, the combination within 1e-14 sum|delta_j b_j| per component, atoms of mass 0 bit for bit."""
    m = 3
    rng = np.random.default_rng(1000 + n)
    xs = [rng.normal(size=(n, 3)) for _ in range(5)]
    gs = [rng.normal(size=(n, 3)) * 10.0 for _ in range(5)]
    mass = np.ones(n)
    if n > 1:
        mass[rng.choice(n, size=max(1, n // 7), replace=False)] = 0.0
    ctx = B.HipContext(n, np.array([5.0, 5.0, 5.0]))
    one = _drive(ctx, n, m, xs, gs, mass)
    two = _drive(ctx, n, m, xs, gs, mass)
    ctx.close()
    # the basis the object holds after four advances: ring slots (0, 1, 2) <- pairs (4, 2, 3), gradients of fixed atoms zeroed
    free = np.repeat(mass > 0, 3)
    g_eff = [np.where(free, g.ravel(), 0.0) for g in gs]
    x_flat = [x.ravel() for x in xs]
    s = {k: np.where(free, x_flat[k] - x_flat[k - 1], 0.0) for k in (2, 3, 4)}
    y = {k: g_eff[k] - g_eff[k - 1] for k in (2, 3, 4)}
    basis = [s[4], s[2], s[3], y[4], y[2], y[3], g_eff[4]]
    for a in range(7):
        for b in range(a, 7):
            prod = basis[a] * basis[b]
            exact, scale = math.fsum(prod.tolist()), float(np.abs(prod).sum())
            assert abs(one['gram'][a, b] - exact) <= 1e-13 * scale, (a, b)
            assert one['gram'][a, b] == one['gram'][b, a]
    last = one['blocks'][-1]
    assert last[3] == np.abs(g_eff[4]).max()
    assert last[2] == one['gram'][6, 6]
    # bit for bit
    assert one['blocks'] == two['blocks'] and one['after_trial'] == two['after_trial']
    for key in ('gram', 'delta', 'direction', 'trial'):
        assert np.array_equal(one[key], two[key]), key
    # the combination
    delta = one['delta']
    want = sum(delta[j] * basis[j] for j in range(7))
    bound = sum(np.abs(delta[j] * basis[j]) for j in range(7))
    assert np.all(np.abs(one['direction'].ravel() - want) <= 1e-14 * bound)
    # g.d comes from the matrix: within the rounding of its terms delta_j (g . b_j), each bounded by |delta_j| |g| |b_j|
    terms = sum(abs(delta[j]) * np.linalg.norm(basis[j]) for j in range(7)) * np.linalg.norm(g_eff[4])
    assert abs(last[1] - float(np.dot(g_eff[4], want))) <= 1e-12 * terms
    # the trial: x_prev + a d, fixed atoms bit for bit
    a = one['after_trial'][6]
    dmax = math.sqrt(float((one['direction'] ** 2).sum(axis=1).max()))
    assert a == pytest.approx(min(1.0, 0.1 / dmax), rel=1e-14)
    assert one['after_trial'][0] == 0.0
    assert np.array_equal(one['trial'][mass == 0], xs[4][mass == 0])
    moved = one['trial'] - xs[4]
    assert np.abs(moved - a * one['direction']).max() <= 4 * np.spacing(np.abs(xs[4]).max() + 0.1)


def test_step_cap_moves_the_farthest_atom_by_max_step():
    """A direction (d = -g after begin) whose largest atom displacement at alpha = 1 is 0.35 nm: the trial moves that atom max_step,
    to the rounding of the coordinates it is added to (three components, each within one spacing of |x| <= 4)."""
    n = 341
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 4.0, size=(n, 3))
    g = rng.normal(size=(n, 3))
    g *= 0.35 / np.linalg.norm(g, axis=1).max()
    ctx = B.HipContext(n, np.array([5.0, 5.0, 5.0]))
    out = _drive(ctx, n, 3, [x], [g], max_step=0.1)
    ctx.close()
    far = int(np.argmax(np.linalg.norm(g, axis=1)))
    moved = np.linalg.norm(out['trial'] - x, axis=1)
    assert abs(moved[far] - 0.1) <= 3 * np.spacing(4.0)
    assert moved.max() <= 0.1 + 3 * np.spacing(4.0)
    assert out['after_trial'][6] == pytest.approx(0.1 / 0.35, rel=1e-14)
    assert np.array_equal(out['direction'], -g)


# ---------------------------------------------------------------------------------------------- 2. direction

def _history(n3, rng, mirrored=None):
    """x_k and g_k = A x_k (A symmetric positive definite, condition number 100), five points; `mirrored`: the pair that ends at that
    point gets y = -A s."""
    q, _ = np.linalg.qr(rng.normal(size=(n3, n3)))
    A = (q * np.geomspace(1.0, 100.0, n3)) @ q.T
    xs = [rng.normal(size=n3)]
    for _ in range(4):
        xs.append(xs[-1] + 0.3 * rng.normal(size=n3))
    gs = [A @ x for x in xs]
    if mirrored is not None:
        shift = 2.0 * (gs[mirrored] - gs[mirrored - 1])
        for k in range(mirrored, 5):
            gs[k] = gs[k] - shift
    return xs, gs


def _restated(xs, gs, m, dtype):
    lb = GramLBFGS(xs[0].size, memory=m, dtype=dtype)
    lb.begin(xs[0], gs[0])
    for x, g in zip(xs[1:], gs[1:]):
        lb.advance(x, g)
    return lb


def test_direction_against_the_extended_precision_restatement():
    """begin + 4 advances at n = 341, m = 3 (the ring wraps).  Bound: 10 x the distance of the fp64 numpy restatement from the
    np.longdouble one, measured here (floor 1e-12 |d|) -- another order of summation must not fail.
    Measured on an MI355X: device - longdouble = 1.7e-16 |d|, fp64 numpy - longdouble = 4.7e-16 |d| (the floor decides)."""
    n, m = 341, 3
    xs, gs = _history(3 * n, np.random.default_rng(2024))
    exact = _restated(xs, gs, m, np.longdouble)
    fp64 = _restated(xs, gs, m, np.float64)
    d_exact = np.asarray(exact.d, dtype=np.longdouble)
    own = float(np.linalg.norm(np.asarray(fp64.d, dtype=np.longdouble) - d_exact))
    size = float(np.linalg.norm(d_exact))
    assert own <= 1e-10 * size                      # the history is well conditioned
    ctx = B.HipContext(n, np.array([5.0, 5.0, 5.0]))
    got = _drive(ctx, n, m, [x.reshape(n, 3) for x in xs], [g.reshape(n, 3) for g in gs])
    ctx.close()
    dist = float(np.linalg.norm(got['direction'].ravel().astype(np.longdouble) - d_exact))
    print('direction: device - longdouble = %.3e |d|, fp64 numpy - longdouble = %.3e |d|' % (dist / size, own / size))
    assert dist <= max(10.0 * own, 1e-12 * size)
    assert got['stats']['dropped'] == 0 and got['stats']['in_use'] == 3 and got['stats']['pairs'] == 4


def test_a_pair_without_curvature_is_dropped_on_the_device():
    n, m = 341, 3
    xs, gs = _history(3 * n, np.random.default_rng(77), mirrored=2)
    ref = _restated(xs, gs, m, np.longdouble)
    assert ref.dropped == 1 and ref.valid == [True, False, True]
    ctx = B.HipContext(n, np.array([5.0, 5.0, 5.0]))
    got = _drive(ctx, n, m, [x.reshape(n, 3) for x in xs], [g.reshape(n, 3) for g in gs])
    ctx.close()
    assert got['stats']['dropped'] == 1 and got['stats']['in_use'] == 2
    assert [b[4] for b in got['blocks']] == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert got['delta'][1] == 0.0 and got['delta'][4] == 0.0           # slot 1 holds the dropped pair
    d_exact = np.asarray(ref.d, dtype=np.float64)
    assert np.linalg.norm(got['direction'].ravel() - d_exact) <= 1e-10 * np.linalg.norm(d_exact)


# ---------------------------------------------------------------------------------------------- 3 .. 8: end to end

@functools.lru_cache(maxsize=None)
def water():
    c = tip3p_box(8)
    c['start'] = c['positions'] + np.random.default_rng(11).normal(scale=0.01, size=c['positions'].shape)
    return c


def water_context(c, integrator=None, mass=None):
    """RESPASystem + DampedSmoothedForce outer force, as tests/test_gpu_api.py builds it: all groups sum to bonds + angles + the
    damped total (the near force of group 1 and its negative in group 31 cancel)."""
    case = dict(c, mass=c['mass'] if mass is None else mass)
    system = system_from_arrays(case, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    outer = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, 1.0 * unit.nanometers, 0.9 * unit.nanometers).importFrom(nb)
    outer.setForceGroup(2)
    outer.addTo(respa)
    context = openmm.Context(respa, integrator or openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    context.setPositions(c['start'] * unit.nanometers)
    context.setVelocities(c['velocities'])
    return context


def oracle_energy_forces(c, x):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    dd = O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1)
    e2, f2 = O.pair_eval(dd, x, c['box'], c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'])[:2]
    eb, fb = O.harmonic_bonds(c['bonds'], c['bond_r0'], c['bond_k'], x, c['box'])
    ea, fa = O.harmonic_angles(c['angles'], c['angle_theta0'], c['angle_k'], x, c['box'])
    return e2 + eb + ea, f2 + fb + fa


def positions_of(context):
    return context.getState(getPositions=True).getPositions(asNumpy=True)._value


def test_flexible_water_end_to_end():
    c = water()
    context = water_context(c)
    e_start = context.getState(getEnergy=True).getPotentialEnergy()._value
    openmm.LocalEnergyMinimizer.minimize(context, 10, 0)
    x = positions_of(context)
    e_ref, f_ref = oracle_energy_forces(c, x)
    rms = math.sqrt(float((f_ref ** 2).mean()))
    print('flexible water: oracle RMS force at the minimum %.4f kJ/mol/nm, energy %.6f -> %.6f' % (rms, e_start, e_ref))
    assert rms <= 10.0
    state = context.getState(getEnergy=True, getVelocities=True)
    assert state.getPotentialEnergy()._value == pytest.approx(e_ref, rel=1e-10)
    assert e_ref < e_start
    assert np.array_equal(state.getVelocities(asNumpy=True)._value, c['velocities'])
    assert context._engine.time == 0.0


class Trace(openmm.MinimizationReporter):
    def __init__(self, stop_at=None):
        self.iterations, self.energies, self.stop_at = [], [], stop_at

    def report(self, iteration, x, grad, args):
        self.iterations.append(iteration)
        self.energies.append(args['system energy'])
        return iteration == self.stop_at


def _cpu_trace(c, scale=None):
    energies = []

    def fun(x):
        e, f = oracle_energy_forces(c, x)
        if scale is not None:
            f = f * scale
        return e, -f.ravel()
    minimize_ref(fun, c['start'].ravel(), tolerance=10.0, max_iterations=5, reporter=lambda it, x, g, e: energies.append(e) and False)
    return np.array(energies)


def test_iteration_trace_against_the_oracle_driven_restatement():
    """Five iterations from the same start: the energies the reporter sees against tests/minimize_ref.py driven by the oracle's energies
    and forces.  Bound: 10 x the largest relative energy difference between two CPU runs, the second with the oracle's forces
    multiplied by 1 + 1e-9 xi (xi uniform in [-1, 1], seeded; 1e-9 is the project's force-parity bar), measured in this test.
    Measured on an MI355X: GPU - CPU = 3.5e-14 relative; CPU with shaken forces - CPU = 1.5e-9 relative (bound 1.5e-8)."""
    c = water()
    plain = _cpu_trace(c)
    xi = np.random.default_rng(9).uniform(-1.0, 1.0, size=c['start'].shape)
    shaken = _cpu_trace(c, 1.0 + 1e-9 * xi)
    assert len(plain) == len(shaken) == 5
    own = float(np.abs(shaken / plain - 1.0).max())
    context = water_context(c)
    trace = Trace()
    openmm.LocalEnergyMinimizer.minimize(context, 10, 5, trace)
    assert trace.iterations == [0, 1, 2, 3, 4]
    gpu = float(np.abs(np.array(trace.energies) / plain - 1.0).max())
    print('trace: GPU - CPU = %.3e relative, CPU with forces shaken by 1e-9 - CPU = %.3e relative' % (gpu, own))
    assert gpu <= 10.0 * own
    # a reporter that returns True stops the minimisation there
    context.setPositions(c['start'] * unit.nanometers)
    stopping = Trace(stop_at=2)
    openmm.LocalEnergyMinimizer.minimize(context, 10, 0, stopping)
    assert stopping.iterations == [0, 1, 2]
    assert stopping.energies == pytest.approx(trace.energies[:3], rel=1e-12)


def test_bonds_and_angles_only():
    """A stretched 30-atom zig-zag chain of harmonic bonds and angles: no pair force, hence no neighbour list, in this run."""
    n, r0, theta0 = 30, 0.15, 1.911
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.011)
    system.setDefaultPeriodicBoxVectors((20.0, 0, 0), (0, 20.0, 0), (0, 0, 20.0))
    bonds, angles = openmm.HarmonicBondForce(), openmm.HarmonicAngleForce()
    for i in range(n - 1):
        bonds.addBond(i, i + 1, r0, 250000.0)
    for i in range(n - 2):
        angles.addAngle(i, i + 1, i + 2, theta0, 400.0)
    system.addForce(bonds)
    system.addForce(angles)
    half = 0.5 * theta0
    x = np.zeros((n, 3))
    x[:, 0] = 5.0 + 1.1 * r0 * math.sin(half) * np.arange(n)
    x[:, 1] = 5.0 + 1.1 * r0 * math.cos(half) * (np.arange(n) % 2)
    x[:, 2] = 5.0
    x += np.random.default_rng(3).normal(scale=0.002, size=x.shape)
    sim = app.Simulation(app.Topology(n), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(x * unit.nanometers)
    engine = sim.context._engine
    assert not [pid for entry in engine.entries for pid in entry.pair_ids]
    info = engine.minimize(10.0, 0, None)
    assert info['reason'] == 'converged'
    state = sim.context.getState(getPositions=True, getForces=True)
    f = state.getForces(asNumpy=True)._value
    assert math.sqrt(float((f ** 2).mean())) <= 10.0
    got = state.getPositions(asNumpy=True)._value
    assert np.abs(np.linalg.norm(got[1:] - got[:-1], axis=1) - r0).max() < 1e-3


def test_atoms_of_mass_zero_stay():
    c = water()
    mass = c['mass'].copy()
    mass[:30] = 0.0                     # molecules 0 .. 9
    context = water_context(c, mass=mass)
    info = context._engine.minimize(10.0, 0, None)
    assert info['reason'] == 'converged'
    x = positions_of(context)
    assert np.array_equal(x[:30], c['start'][:30])
    assert np.abs(x[30:] - c['start'][30:]).max() > 1e-4
    _, f_ref = oracle_energy_forces(c, x)
    assert math.sqrt(float((f_ref[30:] ** 2).mean())) <= 10.0          # the criterion counts the free components only


def test_rigid_water_with_constraints(spcfw):
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic', rigidWater=True)
    assert system.getNumConstraints() == 3 * 512
    nb = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb).addTo(system)
    integrator = atomsmm.GlobalThermostatIntegrator(2 * unit.femtoseconds, atomsmm.VelocityVerletPropagator())
    tolerance = integrator.getConstraintTolerance()
    sim = app.Simulation(app.Topology(len(spcfw['positions'])), system, integrator, openmm.Platform.getPlatformByName('HIP'))
    start = spcfw['positions'] + np.random.default_rng(11).normal(scale=0.01, size=spcfw['positions'].shape)
    sim.context.setPositions(start * unit.nanometers)
    sim.context.applyConstraints()
    e_projected = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy(maxIterations=200)
    x = positions_of(sim.context)
    pairs = np.array([[i, j] for i, j, _ in system._constraints])
    dist = np.array([d for _, _, d in system._constraints])
    error = np.abs(np.linalg.norm(x[pairs[:, 0]] - x[pairs[:, 1]], axis=1) / dist - 1.0).max()
    e_after = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('rigid water: constraint error %.2e (tolerance %.1e), energy %.3f -> %.3f' % (error, tolerance, e_projected, e_after))
    assert error <= tolerance
    assert e_after < e_projected
    sim.context.setVelocitiesToTemperature(300 * unit.kelvin, 4)
    sim.step(2)
    sim.context._engine.ctx.check()


def test_hand_over_to_dynamics():
    """Minimise, then step at once: the trajectory equals the oracle's RESPA from the minimised positions (bars of
    tests/test_gpu_api.py) -- which it cannot if the neighbour lists missed the moves of the minimiser."""
    c = water()
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
    context = water_context(c, integrator=integrator)
    openmm.LocalEnergyMinimizer.minimize(context, 10, 40)
    x_min = positions_of(context)
    assert np.abs(x_min - c['start']).max() > 1e-3
    integrator.step(2)
    cpu = RespaCPU(dict(c, positions=x_min), dt=0.001)
    cpu.step(2)
    state = context.getState(getPositions=True, getVelocities=True)
    assert np.abs(state.getPositions(asNumpy=True)._value - cpu.x).max() < 1e-10
    assert np.abs(state.getVelocities(asNumpy=True)._value - cpu.v).max() < 1e-9


def test_several_ranks_are_refused():
    from atomsmm_amd.engine import LocalWorld
    c = water()

    def job(rank):
        context = water_context(c)
        with pytest.raises(InputError, match='single rank'):
            context._engine.minimize()
        return True
    assert LocalWorld(2).run(job) == [True, True]
