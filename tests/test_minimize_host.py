"""CPU tests of the energy minimiser: the Gram-matrix form of L-BFGS (tests/minimize_ref.py, the numpy restatement of
csrc/minimize.hip) against the textbook recursion, the driver on a convex quadratic, and the Python surface
(LocalEnergyMinimizer, MinimizationReporter, Simulation.minimizeEnergy) over a context that stands in for the HIP library."""
import numpy as np
import pytest

from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.utils import InputError
from fake_backend import RecordingContext
from minimize_ref import GramLBFGS, minimize, two_loop


def spd(n3, cond, rng):
    q, _ = np.linalg.qr(rng.normal(size=(n3, n3)))
    return (q * np.geomspace(1.0, cond, n3)) @ q.T


@pytest.mark.parametrize('m', [1, 3, 8])
def test_gram_form_gives_the_two_loop_direction(m):
    """Random histories with s.y > 0 (y = A s, A symmetric positive definite), n = 5 atoms, more pairs than the ring holds."""
    rng = np.random.default_rng(100 + m)
    n3 = 15
    A = spd(n3, 50.0, rng)
    lb = GramLBFGS(n3, memory=m)
    x = rng.normal(size=n3)
    lb.begin(x, A @ x)
    assert np.allclose(lb.d, -(A @ x), rtol=0, atol=0)           # no history: steepest descent
    pairs = []
    for step in range(m + 3):
        x_new = x + 0.3 * rng.normal(size=n3)
        pairs.append((x_new - x, A @ x_new - A @ x))
        x = x_new
        lb.advance(x, A @ x)
        want = two_loop(pairs[-m:], A @ x)
        assert lb.in_use == min(m, step + 1) and lb.dropped == 0
        assert np.abs(lb.d - want).max() <= 1e-11 * np.abs(want).max()
        assert lb.gd == pytest.approx(np.dot(A @ x, want), rel=1e-9) and lb.gd < 0


def test_a_pair_without_curvature_is_dropped():
    rng = np.random.default_rng(7)
    n3, m = 15, 3
    A = spd(n3, 20.0, rng)
    lb = GramLBFGS(n3, memory=m)
    xs = [rng.normal(size=n3)]
    for _ in range(3):
        xs.append(xs[-1] + 0.3 * rng.normal(size=n3))
    gs = [A @ x for x in xs]
    gs[2] = gs[1] - (gs[2] - gs[1])              # the second pair gets y = -A s: s.y < 0
    lb.begin(xs[0], gs[0])
    for x, g in zip(xs[1:], gs[1:]):
        lb.advance(x, g)
    assert lb.dropped == 1 and lb.in_use == 2 and lb.valid == [True, False, True]
    kept = [(xs[1] - xs[0], gs[1] - gs[0]), (xs[3] - xs[2], gs[3] - gs[2])]
    want = two_loop(kept, gs[3])
    assert np.abs(lb.d - want).max() <= 1e-11 * np.abs(want).max()


def test_driver_reaches_the_minimum_of_a_convex_quadratic():
    rng = np.random.default_rng(3)
    n3 = 30
    A = spd(n3, 100.0, rng)
    centre = rng.normal(size=n3)
    seen = []

    def fun(x):
        return 0.5 * float((x - centre) @ A @ (x - centre)), A @ (x - centre)
    out = minimize(fun, centre + rng.normal(size=n3), tolerance=1e-8, reporter=lambda it, x, g, e: seen.append((it, e)) and False)
    assert out['reason'] == 'converged'
    assert np.abs(out['x'] - centre).max() < 1e-8
    assert [it for it, _ in seen] == list(range(out['iterations']))
    assert all(b <= a for (_, a), (_, b) in zip(seen, seen[1:]))          # Armijo: the energy never rises
    # atoms held fixed do not move, and the tolerance counts the free components only
    free = np.repeat(np.arange(10) >= 2, 3)
    start = centre + rng.normal(size=n3)
    # (the minimum over the free atoms has an energy of order 1, whose rounding, 1e-16, resolves gradients of order 1e-7 only:
    # the Armijo test cannot see smaller ones, so this run asks for 1e-5)
    out = minimize(fun, start, tolerance=1e-5, free=free)
    assert np.array_equal(out['x'][~free], start[~free]) and out['reason'] == 'converged'
    assert np.sqrt(np.mean((A @ (out['x'] - centre))[free] ** 2)) <= 1e-5
    # the cap: no atom moves farther than max_step in one trial
    lb = GramLBFGS(n3, max_step=0.1)
    lb.begin(start, 100.0 * (A @ (start - centre)))
    moved = np.linalg.norm((lb.trial(1.0) - start).reshape(-1, 3), axis=1)
    assert moved.max() == pytest.approx(0.1, rel=1e-12)


def test_driver_stops_at_max_iterations_and_at_the_reporter():
    A = np.diag(np.geomspace(1.0, 1e4, 12))

    def fun(x):
        return 0.5 * float(x @ A @ x), A @ x
    out = minimize(fun, np.ones(12), tolerance=1e-12, max_iterations=3)
    assert (out['iterations'], out['reason']) == (3, 'max iterations')
    out = minimize(fun, np.ones(12), tolerance=1e-12, reporter=lambda it, x, g, e: it == 2)
    assert (out['iterations'], out['reason']) == (3, 'reporter')


# ---- the Python surface, over a stand-in for the HIP library that serves the minimiser's calls with the numpy restatement

class MinimizingRecorder(RecordingContext):
    """RecordingContext + harmonic bond-list sets that are evaluated (numpy) + the amm_min_* entry points (GramLBFGS)."""

    def bonded_add_terms(self, fid, kind, idx, params, periodic=False, desc=None):
        super().bonded_add_terms(fid, kind, idx, params, periodic, desc)
        assert kind == 0          # BOND_HARMONIC
        self.terms = getattr(self, 'terms', {})
        self.terms.setdefault(fid, []).append((np.asarray(idx).reshape(-1, 2), np.asarray(params).reshape(-1, 2)))

    def force_eval(self, fid, pos, force, accumulate=False, energy=None):
        super().force_eval(fid, pos, force, accumulate)
        x, f = pos.numpy(), np.zeros((self.n, 3))
        e = 0.0
        for idx, par in self.terms[fid]:
            d = x[idx[:, 0]] - x[idx[:, 1]]
            r = np.linalg.norm(d, axis=1)
            e += float((0.5 * par[:, 1] * (r - par[:, 0]) ** 2).sum())
            pull = (-par[:, 1] * (r - par[:, 0]) / r)[:, None] * d
            np.add.at(f, idx[:, 0], pull)
            np.add.at(f, idx[:, 1], -pull)
        force.numpy()[...] = (force.numpy() if accumulate else 0.0) + f
        if energy is not None:
            energy[0] += e

    def positions_changed(self):
        self.calls.append(('positions_changed',))

    def set_option(self, name, value):
        pass

    def min_create(self, scalars, mass=None, memory=8, max_step=0.1, force_input=True):
        free = None if mass is None else np.repeat(mass.numpy() > 0, 3)
        self.lb, self.scal, self.sign = GramLBFGS(3 * self.n, memory, free, max_step), scalars, -1.0 if force_input else 1.0
        self.calls.append(('min_create', memory, max_step))
        return 0

    def _publish(self):
        lb = self.lb
        self.scal[1], self.scal[2], self.scal[3] = float(lb.gd), float(lb.gg), float(lb.gmax)
        self.scal[4], self.scal[5], self.scal[7] = float(lb.newest_dropped), float(lb.in_use), float(lb.dmax2)

    def min_begin(self, mid, x=None, g=None):
        if x is None:
            self.lb.restart()
        else:
            self.lb.begin(x.numpy().ravel(), self.sign * g.numpy().ravel())
        self._publish()

    def min_advance(self, mid, x, g):
        self.lb.advance(x.numpy().ravel(), self.sign * g.numpy().ravel())
        self._publish()

    def min_trial(self, mid, alpha, x_out):
        self.scal[0], self.scal[6] = 0.0, float(self.lb.step_factor(alpha))
        x_out.numpy()[...] = self.lb.trial(alpha).reshape(-1, 3)

    def min_scalars(self, mid):
        return self.scal.tolist()

    def min_stats(self, mid):
        return dict(pairs=0, trials=0, dropped=self.lb.dropped, restarts=self.lb.restarts, resets=self.lb.resets, in_use=0, memory=self.lb.m)

    def min_release(self, mid):
        self.calls.append(('min_release', mid))


@pytest.fixture
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(MinimizingRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def stretched_chain(n=30, r0=0.15, k=250000.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.0)
    system.setDefaultPeriodicBoxVectors((20.0, 0, 0), (0, 20.0, 0), (0, 0, 20.0))
    bonds = openmm.HarmonicBondForce()
    for i in range(n - 1):
        bonds.addBond(i, i + 1, r0, k)
    system.addForce(bonds)
    rng = np.random.default_rng(5)
    positions = np.zeros((n, 3))
    positions[:, 0] = 1.0 + 1.1 * r0 * np.arange(n)
    positions += rng.normal(scale=0.005, size=positions.shape)
    return system, positions


def bond_lengths(x):
    return np.linalg.norm(x[1:] - x[:-1], axis=1)


def test_minimize_energy_through_the_python_surface(recorder):
    system, positions = stretched_chain()
    sim = app.Simulation(app.Topology(len(positions)), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(positions * unit.nanometers)
    sim.context.setVelocities(np.full(positions.shape, 0.25))
    sim.minimizeEnergy()
    x = sim.context._engine.x.numpy()
    assert np.abs(bond_lengths(x) - 0.15).max() < 1e-3
    assert np.array_equal(sim.context._engine.v.numpy(), np.full(positions.shape, 0.25)) and sim.context._engine.time == 0.0
    rec = recorder[-1]
    assert ('min_create', 8, 0.1) in rec.calls and rec.calls[-1][0] == 'min_release'
    trials = sum(1 for c in rec.calls if c[0] == 'positions_changed')
    assert trials >= 2          # one after setPositions, one per trial


class Recording(openmm.MinimizationReporter):
    def __init__(self, stop_at=None):
        self.seen, self.stop_at = [], stop_at

    def report(self, iteration, x, grad, args):
        assert len(x) == len(grad) == 90
        self.seen.append((iteration, args['system energy'], dict(args)))
        return iteration == self.stop_at


def test_reporter_and_argument_handling(recorder):
    assert openmm.MinimizationReporter().report(0, [], [], {}) is False
    system, positions = stretched_chain()
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(positions)
    reporter = Recording()
    openmm.LocalEnergyMinimizer.minimize(context, 10 * unit.kilojoules_per_mole / unit.nanometer, 4, reporter)
    assert [s[0] for s in reporter.seen] == [0, 1, 2, 3]
    energies = [s[1] for s in reporter.seen]
    assert all(b <= a for a, b in zip(energies, energies[1:]))
    assert set(reporter.seen[0][2]) == {'system energy', 'restraint energy', 'restraint strength', 'max constraint error'}
    assert reporter.seen[0][2]['restraint energy'] == 0.0
    # stops where the reporter says so
    context.setPositions(positions)
    stopping = Recording(stop_at=2)
    openmm.LocalEnergyMinimizer.minimize(context, reporter=stopping)
    assert [s[0] for s in stopping.seen] == [0, 1, 2]
    # units: 1 kcal/mol/angstrom = 41.84 kJ/mol/nm reaches the engine as that number; a bare number is kJ/mol/nm
    got = []
    context._engine.minimize = lambda tolerance, max_iterations, reporter: got.append((tolerance, max_iterations, reporter))
    openmm.LocalEnergyMinimizer.minimize(context, 1 * unit.kilocalories_per_mole / unit.angstrom, maxIterations=7)
    openmm.LocalEnergyMinimizer.minimize(context, 2.5)
    assert got[0] == (pytest.approx(41.84), 7, None) and got[1] == (2.5, 0, None)
    with pytest.raises(TypeError):
        openmm.LocalEnergyMinimizer.minimize(context, 1 * unit.nanometers)
    with pytest.raises(openmm.OpenMMException):
        openmm.LocalEnergyMinimizer.minimize(context, -1.0)
    with pytest.raises(openmm.OpenMMException):
        openmm.LocalEnergyMinimizer.minimize(context, 10.0, -2)
    with pytest.raises(TypeError):
        openmm.LocalEnergyMinimizer.minimize(context, 10.0, 0, reporter=object())


def test_aliases_carry_the_minimiser():
    import simtk.openmm as simtk_openmm
    assert simtk_openmm.LocalEnergyMinimizer is openmm.LocalEnergyMinimizer
    assert simtk_openmm.MinimizationReporter is openmm.MinimizationReporter
    assert hasattr(simtk_openmm.app.Simulation, 'minimizeEnergy')


def test_several_ranks_are_refused(recorder):
    system, positions = stretched_chain()

    def job(rank):
        context = openmm.Context(system, openmm.VerletIntegrator(0.001))
        with pytest.raises(InputError, match='single rank'):
            context._engine.minimize()
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
