"""CPU tests of constant-pressure runs on the host side: when Engine.step makes the attempts of a MonteCarloBarostat, in which order
it draws its random numbers, how the step size adapts, the Context parameters, what is refused, and -- on an ideal gas, where the
stationary law is known in closed form -- the sign of every term of the acceptance test.  A call recorder that moves molecules
and answers energies from a Python function stands in for the HIP library."""
import math

import numpy as np
import pytest

from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.utils import InputError
from fake_backend import RecordingContext

KT_300 = unit.MOLAR_GAS_CONSTANT_R._value * 300.0
BAR = unit.bar.scale                      # 1 bar in kJ/mol/nm^3 (N_A 1e-25)


class BarostatRecorder(RecordingContext):
    """RecordingContext + the box and molecule entry points (numpy) + energies answered by `energy_of(context)`."""
    energy_of = staticmethod(lambda ctx: 0.0)

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.box = np.array(self.box, dtype=np.float64)
        self.events = []                  # ('run', steps) and ('attempt',) in the order they happened

    def set_option(self, name, value):
        pass

    def positions_changed(self):
        self.calls.append(('positions_changed',))

    def bind_state(self, x, v, mass):
        self.x = x

    def set_box(self, edges):
        self.box = np.array(edges, dtype=np.float64)
        self.calls.append(('set_box', tuple(self.box)))

    def mol_define(self, molecules):
        self.molecules = [list(m) for m in molecules]
        self._flat = np.array([i for m in self.molecules for i in m])
        self._owner = np.repeat(np.arange(len(self.molecules)), [len(m) for m in self.molecules])
        self._count = np.array([len(m) for m in self.molecules], dtype=np.float64)[:, None]
        assert sorted(self._flat) == list(range(self.n))

    def mol_scale(self, x, scale, saved=None):
        self.events.append(('attempt',))
        xs = x.numpy()
        if saved is not None:
            saved.numpy()[...] = xs
        sums = np.zeros((len(self.molecules), 3))
        np.add.at(sums, self._owner, xs[self._flat])
        xs[self._flat] += (np.asarray(scale) - 1.0) * (sums / self._count)[self._owner]

    def copy(self, dst, src):
        dst.copy_(src)

    def run_ops(self, ops, repeat=1):
        super().run_ops(ops, repeat)
        self.events.append(('run', repeat))

    def force_eval(self, fid, pos, force, accumulate=False, energy=None):
        super().force_eval(fid, pos, force, accumulate)
        if energy is not None:
            energy[0] += self.energy_of(self)


@pytest.fixture
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(BarostatRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


class Scripted:
    """Stands in for the barostat's generator: hands out the numbers it is given and counts the draws."""

    def __init__(self, values):
        self.values, self.draws = iter(values), 0

    def random(self):
        self.draws += 1
        return next(self.values)


def gas(n=63, edge=13.8, bonded=False):
    """n single atoms without forces (an ideal gas); bonded: atoms 0 and 1 form one molecule, so that an energy is evaluated."""
    system = openmm.System()
    for _ in range(n):
        system.addParticle(40.0)
    system.setDefaultPeriodicBoxVectors((edge, 0, 0), (0, edge, 0), (0, 0, edge))
    if bonded:
        bonds = openmm.HarmonicBondForce()
        bonds.addBond(0, 1, 0.1, 1000.0)
        system.addForce(bonds)
    positions = np.random.default_rng(1).uniform(0.0, edge, (n, 3))
    return system, positions


def drift(dt=0.001, update_first=True):
    integrator = openmm.CustomIntegrator(dt)
    if update_first:
        integrator.addUpdateContextState()
    integrator.addComputePerDof('x', 'x+dt*v')
    if not update_first:
        integrator.addUpdateContextState()
    return integrator


def context_with(barostat, recorder, **kw):
    system, positions = gas(**kw)
    system.addForce(barostat)
    context = openmm.Context(system, drift())
    context.setPositions(positions)
    return context, recorder[-1]


def test_python_surface():
    import simtk.openmm as simtk_openmm
    assert simtk_openmm.MonteCarloBarostat is openmm.MonteCarloBarostat
    b = openmm.MonteCarloBarostat(1.0 * unit.atmosphere, 300.0 * unit.kelvin)
    assert b.getFrequency() == 25 and b.getRandomNumberSeed() == 0 and not b.usesPeriodicBoundaryConditions()
    assert b.getDefaultPressure().value_in_unit(unit.bar) == pytest.approx(1.01325, rel=1e-12)
    assert b.getDefaultTemperature().value_in_unit(unit.kelvin) == 300.0
    assert b.Pressure() == 'MonteCarloPressure' and b.Temperature() == 'MonteCarloTemperature'
    b = openmm.MonteCarloBarostat(2.0, 310.0, 7)
    assert (b.getDefaultPressure()._value, b.getDefaultTemperature()._value, b.getFrequency()) == (2.0, 310.0, 7)
    b.setDefaultPressure(3.0 * unit.bar)
    b.setDefaultTemperature(280.0)
    b.setFrequency(0)
    b.setRandomNumberSeed(12)
    assert (b.getDefaultPressure()._value, b.getDefaultTemperature()._value, b.getFrequency(), b.getRandomNumberSeed()) == (3.0, 280.0, 0, 12)
    with pytest.raises(openmm.OpenMMException):
        b.setFrequency(-1)


def test_attempts_come_right_before_every_fourth_step(recorder):
    barostat = openmm.MonteCarloBarostat(1.0, 300.0, 4)
    barostat.setRandomNumberSeed(5)
    context, rec = context_with(barostat, recorder)
    context.getIntegrator().step(7)
    first = list(rec.events)
    context.getIntegrator().step(5)
    done, before = 0, []
    for event in rec.events:
        if event[0] == 'run':
            done += event[1]
        else:
            before.append(done + 1)             # the step the attempt comes right before
    assert before == [4, 8, 12] and done == 12
    assert sum(e[1] for e in first if e[0] == 'run') == 7 and sum(1 for e in first if e[0] == 'attempt') == 1
    assert context._engine.barostat_stats['attempts'] == 3
    assert context._engine.time == pytest.approx(0.012)
    # the steps between two attempts go to the library as whole chunks: no chunk of one step where four belong together
    assert [e[1] for e in rec.events if e[0] == 'run'] == [3, 4, 4, 1]


def test_second_number_is_drawn_only_when_w_is_positive(recorder):
    barostat = openmm.MonteCarloBarostat(1.0, 300.0, 1)
    context, rec = context_with(barostat, recorder, bonded=True)
    engine = context._engine
    # energies per attempt (before, after): downhill by far, uphill by far, uphill by 1 kJ/mol at an unchanged volume (w = 1)
    energies = iter([0.0, -1e6, 0.0, 1e6, 0.0, 1.0])
    rec.energy_of = lambda ctx: next(energies)
    rng = engine._baro_rng = Scripted([0.75, 0.25, 0.5, 0.5, 0.5, math.exp(-1.0 / KT_300) - 1e-3])
    box0 = engine.box.copy()
    engine.step(1)
    assert rng.draws == 1 and engine.barostat_log[-1][0] and engine.barostat_log[-1][2] is None      # w < 0: accepted, no second draw
    box1, x1 = engine.box.copy(), engine.x.clone()
    assert box1[0] == pytest.approx(box0[0] * (1.0 + 0.01 * 0.5) ** (1.0 / 3.0), rel=1e-14)
    engine.step(1)
    assert rng.draws == 3 and not engine.barostat_log[-1][0] and engine.barostat_log[-1][2] == 0.5     # w > 0, u2 > exp(-w/kT): rejected
    assert np.array_equal(engine.box, box1) and np.array_equal(rec.box, box1)                           # the old box, bit for bit
    moved = engine.x - x1
    assert np.array_equal(moved.numpy(), np.zeros_like(moved.numpy()))        # (v = 0: the step itself moves nothing) the old bits
    engine.step(1)
    assert rng.draws == 5 and engine.barostat_log[-1][0] and engine.barostat_log[-1][2] is not None    # w > 0, u2 < exp(-w/kT): accepted
    assert engine.barostat_stats == dict(attempts=3, accepted=2)


def test_step_size_adaptation(recorder):
    barostat = openmm.MonteCarloBarostat(1.0, 300.0, 1)
    context, rec = context_with(barostat, recorder, bonded=True)
    engine = context._engine
    volume = float(np.prod(engine.box))
    flip = {'sign': +1.0, 'k': 0}

    def energy(ctx):                        # every second evaluation is the one after the move: +-1e9 above the one before it
        flip['k'] += 1
        return flip['sign'] * 1e9 if flip['k'] % 2 == 0 else 0.0
    rec.energy_of = energy
    # u1 = 0.5: the volume does not change, whatever the step size; u2 = 0.5 rejects every uphill move
    engine._baro_rng = Scripted(iter(lambda: 0.5, None))
    engine.step(9)
    assert engine._baro_scale == 0.01 * volume
    engine.step(1)                          # ten attempts, none accepted: / 1.1
    assert engine._baro_scale == pytest.approx(0.01 * volume / 1.1, rel=1e-15) and engine._baro_window == [0, 0]
    flip['sign'] = -1.0
    engine.step(10)                         # ten attempts, all accepted: x 1.1
    assert engine._baro_scale == pytest.approx(0.01 * volume, rel=1e-14)
    engine.step(400)                        # 1.1^36 > 30: the cap of 0.3 V is reached and held
    assert engine._baro_scale == 0.3 * volume
    assert engine.barostat_stats == dict(attempts=420, accepted=410)
    # five of ten: between 25 % and 75 % nothing changes and the counters run on
    engine._baro_scale, engine._baro_window = 0.02 * volume, [0, 0]
    for sign in [+1.0, -1.0] * 5:
        flip['sign'] = sign
        engine.step(1)
    assert engine._baro_scale == 0.02 * volume and engine._baro_window == [10, 5]


def test_parameters_and_switches(recorder):
    barostat = openmm.MonteCarloBarostat(1.0, 300.0, 1)
    context, rec = context_with(barostat, recorder)
    engine = context._engine
    assert context.getParameter('MonteCarloPressure') == 1.0 and context.getParameter('MonteCarloTemperature') == 300.0
    n, volume = 63, float(np.prod(engine.box))

    def expected_w(pressure, temperature, u1, volume, scale):
        delta = scale * 2.0 * (u1 - 0.5)
        return pressure * BAR * delta - n * unit.MOLAR_GAS_CONSTANT_R._value * temperature * math.log((volume + delta) / volume)
    engine._baro_rng = Scripted([0.9, 0.999, 0.9, 0.999, 0.9, 0.999])
    engine.step(1)
    assert engine.barostat_log[-1][1] == pytest.approx(expected_w(1.0, 300.0, 0.9, volume, 0.01 * volume), rel=1e-12)
    assert not engine.barostat_log[-1][0]                     # (expanding a gas far below its pressure-volume balance: uphill, u2 ~ 1)
    context.setParameter('MonteCarloPressure', 2.5)
    engine.step(1)
    assert engine.barostat_log[-1][1] == pytest.approx(expected_w(2.5, 300.0, 0.9, volume, 0.01 * volume), rel=1e-12)
    context.setParameter('MonteCarloPressure', 2.5 * unit.bar)   # (a Quantity is a number of bar too: nothing changed)
    context.setParameter('MonteCarloTemperature', 150.0)
    engine.step(1)
    assert engine.barostat_log[-1][1] == pytest.approx(expected_w(2.5, 150.0, 0.9, volume, 0.01 * volume), rel=1e-12)
    assert engine.barostat_stats['attempts'] == 3
    # frequency 0: never
    barostat.setFrequency(0)
    engine.step(50)
    assert engine.barostat_stats['attempts'] == 3
    off = openmm.MonteCarloBarostat(1.0, 300.0, 0)
    context, rec = context_with(off, recorder)
    context.getIntegrator().step(30)
    assert context._engine.barostat_stats['attempts'] == 0 and ('attempt',) not in rec.events


def test_live_box_through_the_context(recorder):
    system, positions = gas(bonded=True)
    context = openmm.Context(system, drift())
    context.setPositions(positions)
    rec, engine = recorder[-1], context._engine
    engine._valid['all'] = True
    context.setPeriodicBoxVectors((14.0, 0, 0), (0, 15.0, 0) * unit.nanometers, openmm.Vec3(0, 0, 16.0))
    assert ('set_box', (14.0, 15.0, 16.0)) in rec.calls and np.array_equal(engine.box, [14.0, 15.0, 16.0])
    assert engine._valid['all'] is False                       # forces are stale
    assert np.array_equal(engine.x.numpy(), positions)         # positions are not touched
    state = context.getState(getPositions=True)
    assert [tuple(v._value) for v in state.getPeriodicBoxVectors()] == [(14.0, 0, 0), (0, 15.0, 0), (0, 0, 16.0)]
    with pytest.raises(InputError, match='only orthorhombic'):
        context.setPeriodicBoxVectors((14.0, 0.1, 0), (0, 15.0, 0), (0, 0, 16.0))
    # setState: the box first, then the positions
    other = openmm.Context(system, drift())
    del recorder[-1].calls[:]
    other.setState(state)
    names = [c[0] for c in recorder[-1].calls]
    assert names.index('set_box') < names.index('positions_changed')
    assert np.array_equal(other._engine.box, [14.0, 15.0, 16.0])


def test_long_range_corrections_follow_the_volume(recorder):
    """The dispersion correction of a NonbondedForce is proportional to 1 / V."""
    system, positions = gas(n=20, edge=4.0)
    nb = openmm.NonbondedForce()
    for _ in range(20):
        nb.addParticle(0.0, 0.3, 0.5)
    nb.setNonbondedMethod(nb.CutoffPeriodic)
    nb.setCutoffDistance(1.0)
    nb.setUseDispersionCorrection(True)
    system.addForce(nb)
    context = openmm.Context(system, drift())
    context.setPositions(positions)
    engine = context._engine
    entry = engine.entries[0]
    c0 = entry.constant
    assert c0 == E.dispersion_correction(np.full(20, 0.3), np.full(20, 0.5), np.full(3, 4.0), 1.0) and c0 < 0
    context.setPeriodicBoxVectors((4.4, 0, 0), (0, 4.0, 0), (0, 0, 5.0))
    fresh = E.dispersion_correction(np.full(20, 0.3), np.full(20, 0.5), np.array([4.4, 4.0, 5.0]), 1.0)
    assert entry.constant == pytest.approx(fresh, rel=1e-14) and entry.constant == pytest.approx(c0 * 64.0 / 88.0, rel=1e-14)
    context.setPeriodicBoxVectors((4.0, 0, 0), (0, 4.0, 0), (0, 0, 4.0))
    assert entry.constant == c0


def test_globals_are_not_kept_on_the_device_next_to_a_barostat(recorder):
    """Device-resident extended variables (AFED) carry 1 / V in the coefficients of their correction polynomials: with a barostat
    the engine waits for such globals instead, so no polynomial can outlive an attempt."""
    context, rec = context_with(openmm.MonteCarloBarostat(1.0, 300.0, 5), recorder)
    rec.expr_eval_scalar = lambda *a: None                 # (a backend that has the scalar kernel)
    assert context._engine.device_globals is False and not context._engine._device_scalars_ok()
    system, positions = gas()
    plain = openmm.Context(system, drift())
    recorder[-1].expr_eval_scalar = lambda *a: None
    assert plain._engine._device_scalars_ok()


def test_refusals(recorder):
    system, positions = gas()
    system.addForce(openmm.MonteCarloBarostat(1.0, 300.0))
    # a program that moves x ahead of its UpdateContextState step
    with pytest.raises(NotImplementedError, match='ahead of its UpdateContextState'):
        openmm.Context(system, drift(update_first=False))
    reads = openmm.CustomIntegrator(0.001)
    reads.addComputePerDof('v', 'v+dt*f/m')
    reads.addUpdateContextState()
    reads.addComputePerDof('x', 'x+dt*v')
    with pytest.raises(NotImplementedError, match='ahead of its UpdateContextState'):
        openmm.Context(system, reads)
    # ... while one that only touches v and globals there is fine, as is one without the step (OpenMM then updates at the start)
    harmless = openmm.CustomIntegrator(0.001)
    harmless.addGlobalVariable('a', 0.0)
    harmless.addComputeGlobal('a', 'a+1')
    harmless.addComputePerDof('v', 'v*0.5')
    harmless.addUpdateContextState()
    harmless.addComputePerDof('x', 'x+dt*v')
    openmm.Context(system, harmless)
    bare = openmm.CustomIntegrator(0.001)
    bare.addComputePerDof('x', 'x+dt*v')
    openmm.Context(system, bare)
    # regulated moves
    regulated = openmm.CustomIntegrator(0.001)
    regulated.addUpdateContextState()
    regulated.addComputePerDof('x', 'x+dt*tanh(v)')
    with pytest.raises(NotImplementedError, match='regulated'):
        openmm.Context(system, regulated)
    # two barostats
    system.addForce(openmm.MonteCarloBarostat(1.0, 300.0))
    with pytest.raises(InputError, match='one MonteCarloBarostat'):
        openmm.Context(system, drift())

    # several ranks: neither a barostat nor a box change
    def job(rank):
        system, positions = gas()
        context = openmm.Context(system, drift())
        with pytest.raises(InputError, match='single rank'):
            context.setPeriodicBoxVectors((14.0, 0, 0), (0, 14.0, 0), (0, 0, 14.0))
        system.addForce(openmm.MonteCarloBarostat(1.0, 300.0))
        with pytest.raises(InputError, match='single rank'):
            openmm.Context(system, drift())
        return True
    assert E.LocalWorld(2).run(job) == [True, True]


def test_ideal_gas_volume_follows_the_gamma_law(recorder):
    """63 atoms without forces at 1 bar and 300 K: the chain's stationary density is V^N exp(-P V / kT), i.e. V ~ Gamma(N + 1, kT / P)
    with mean (N + 1) kT / P.  A wrong sign of the P dV term, of the N kT ln term or of the Metropolis test moves the mean by many
    standard errors (or sends the volume to zero or infinity)."""
    n, attempts = 63, 24000
    barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 1)
    barostat.setRandomNumberSeed(20261017)
    context, rec = context_with(barostat, recorder)
    engine = context._engine
    volumes = np.empty(attempts)
    for k in range(attempts // 1000):
        for j in range(1000):
            engine.step(1)
            volumes[1000 * k + j] = np.prod(engine.box)
        del rec.runs[:], rec.events[:], rec.calls[:]
    assert engine.barostat_stats['attempts'] == attempts
    kept = volumes[attempts // 10:]
    blocks = kept[:len(kept) // 24 * 24].reshape(24, -1).mean(axis=1)
    mean, stderr = blocks.mean(), blocks.std(ddof=1) / math.sqrt(len(blocks))
    expected = (n + 1) * KT_300 / BAR
    rate = engine.barostat_stats['accepted'] / attempts
    print('ideal gas: <V> = %.1f +- %.1f nm^3 (24 blocks), expected %.1f; acceptance %.3f' % (mean, stderr, expected, rate))
    assert abs(mean - expected) <= 5.0 * stderr
    assert stderr < 0.05 * expected                      # (a chain that does not move would pass the line above with a huge error bar)
    assert 0.25 <= rate <= 0.75
