"""CPU tests of OpenMM's stock integrators on the host side: the classes and their accessors, the step program the engine hands to
the library with its `stock_native` switch on (EVAL ; STOCK) and off (the same step from the existing ops), what invalidates it,
what is refused.  A call recorder stands in for the HIP library; the arithmetic is tested on the GPU (test_gpu_stock.py)."""
import math

import numpy as np
import pytest

from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from fake_backend import RecordingContext

KB = unit.BOLTZMANN_CONSTANT_kB._value


class StockRecorder(RecordingContext):
    """RecordingContext + the entry points a stock integrator (and a barostat) needs."""
    has_stock = True

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.stocks = []

    def __getattribute__(self, name):
        # (a recorder of a library without the op: hasattr(ctx, 'stock_define') must be False)
        if name == 'stock_define' and not object.__getattribute__(self, 'has_stock'):
            raise AttributeError(name)
        return object.__getattribute__(self, name)

    def stock_define(self, kind, dt, friction, kT):
        self.stocks.append((kind, dt, friction, kT))
        return len(self.stocks) - 1

    def constraints_set_tolerance(self, tolerance):
        self.constraints = (self.constraints[0], tolerance)
        self.calls.append(('constraints_set_tolerance', tolerance))

    def set_option(self, name, value):
        pass

    def positions_changed(self):
        pass

    def set_box(self, edges):
        self.box = np.array(edges, dtype=np.float64)

    def mol_define(self, molecules):
        self.molecules = molecules

    def mol_scale(self, x, scale, saved=None):
        self.calls.append(('mol_scale',))

    def copy(self, dst, src):
        dst.copy_(src)


class OldLibrary(StockRecorder):
    has_stock = False


@pytest.fixture
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(factory.cls(*a, **k))
        return made[-1]
    factory.cls = StockRecorder
    monkeypatch.setattr(E, '_context_factory', factory)
    made.append(factory)            # made[0]: the factory (to switch the recorder class), made[-1]: the last recorder
    return made


def waters(n_mol=4, constrained=True, edge=3.0, box=True):
    """n_mol three-site molecules with harmonic bonds (a force to evaluate) and, if asked, rigid-triangle constraints."""
    system = openmm.System()
    bonds = openmm.HarmonicBondForce()
    for k in range(n_mol):
        for mass in (15.9994, 1.008, 1.008):
            system.addParticle(mass)
        bonds.addBond(3 * k, 3 * k + 1, 0.1, 1000.0)
        if constrained:
            system.addConstraint(3 * k, 3 * k + 1, 0.1)
            system.addConstraint(3 * k, 3 * k + 2, 0.1)
            system.addConstraint(3 * k + 1, 3 * k + 2, 0.16)
    if box:
        system.setDefaultPeriodicBoxVectors((edge, 0, 0), (0, edge, 0), (0, 0, edge))
    system.addForce(bonds)
    return system


def names(run):
    table = {B.OP_EVAL: 'EVAL', B.OP_KICK: 'KICK', B.OP_MOVE: 'MOVE', B.OP_COPY: 'COPY', B.OP_EXPR: 'EXPR', B.OP_BATH: 'BATH',
             B.OP_SAVE_REF: 'SAVE_REF', B.OP_CONSTRAIN_X: 'CONSTRAIN_X', B.OP_CONSTRAIN_V: 'CONSTRAIN_V', B.OP_STOCK: 'STOCK'}
    return [table[op[0]] for op in run[0]]


def make(kind):
    if kind == 'verlet':
        return openmm.VerletIntegrator(2 * unit.femtoseconds)
    cls = dict(middle=openmm.LangevinMiddleIntegrator, langevin=openmm.LangevinIntegrator, brownian=openmm.BrownianIntegrator)[kind]
    return cls(300 * unit.kelvin, 1 / unit.picosecond, 2 * unit.femtoseconds)


def test_constructors_accessors_and_units():
    import simtk.openmm as simtk_openmm
    for name in ('VerletIntegrator', 'LangevinIntegrator', 'LangevinMiddleIntegrator', 'BrownianIntegrator'):
        assert getattr(simtk_openmm, name) is getattr(openmm, name)
    v = openmm.VerletIntegrator(2 * unit.femtoseconds)
    assert v.getStepSize().value_in_unit(unit.picosecond) == pytest.approx(0.002, rel=1e-15)
    assert v.getConstraintTolerance() == 1e-5 and v.getRandomNumberSeed() == 0
    v.setStepSize(0.001)
    v.setConstraintTolerance(1e-8)
    v.setRandomNumberSeed(7)
    assert (v.getStepSize()._value, v.getConstraintTolerance(), v.getRandomNumberSeed()) == (0.001, 1e-8, 7)
    for cls in (openmm.LangevinIntegrator, openmm.LangevinMiddleIntegrator, openmm.BrownianIntegrator):
        # OpenMM's order: temperature, friction coefficient, step size; plain numbers are K, 1/ps, ps
        a = cls(310 * unit.kelvin, 2 / unit.picosecond, 4 * unit.femtoseconds)
        b = cls(310.0, 2.0, 0.004)
        for i in (a, b):
            assert i.getTemperature().value_in_unit(unit.kelvin) == 310.0
            assert i.getFriction()._value == 2.0 and i.getFriction().unit.dims == (1 / unit.picosecond).unit.dims
            assert i.getStepSize()._value == pytest.approx(0.004, rel=1e-15)
        a.setTemperature(280 * unit.kelvin)
        a.setFriction(5 / unit.picosecond)
        a.setStepSize(1 * unit.femtoseconds)
        assert (a.getTemperature()._value, a.getFriction()._value) == (280.0, 5.0)
        assert a.getStepSize()._value == pytest.approx(0.001, rel=1e-15)
        # friction given per femtosecond: 1/fs = 1000/ps
        assert cls(300.0, 0.001 / unit.femtosecond, 0.001).getFriction()._value == pytest.approx(1.0, rel=1e-12)
        with pytest.raises(openmm.OpenMMException):
            cls(-1.0, 1.0, 0.001)
        with pytest.raises(openmm.OpenMMException):
            cls(300.0, -1.0, 0.001)
    with pytest.raises(openmm.OpenMMException):
        openmm.BrownianIntegrator(300.0, 0.0, 0.001)
    assert not isinstance(openmm.LangevinMiddleIntegrator(300.0, 1.0, 0.002), openmm.CustomIntegrator)
    with pytest.raises(openmm.OpenMMException):
        openmm.LangevinMiddleIntegrator(300.0, 1.0, 0.002).step(1)         # not bound to a context


@pytest.mark.parametrize('kind, stock_kind', [('verlet', 0), ('middle', 1), ('langevin', 2), ('brownian', 3)])
def test_native_step_is_eval_then_stock(recorder, kind, stock_kind):
    integrator = make(kind)
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    ctx = recorder[-1]
    integrator.step(5)
    # (the first step of a Context is a program of its own, as for every compiled program: no force group is known to be stale yet)
    assert [run[1] for run in ctx.runs] == [1, 4]                    # then one call for the rest: the `repeat` path
    assert names(ctx.runs[0]) == names(ctx.runs[1]) == ['EVAL', 'STOCK'] and ctx.runs[0][0] == ctx.runs[1][0]
    (_, group, _, _, _), (_, stock_id, slot, _, _) = ctx.runs[1][0]
    assert ctx.groups[group][0] == slot          # STOCK reads the buffer the EVAL wrote
    friction = 0.0 if kind == 'verlet' else 1.0
    kT = 0.0 if kind == 'verlet' else KB * 300.0
    assert ctx.stocks == [(stock_kind, pytest.approx(0.002, rel=1e-15), friction, pytest.approx(kT, rel=1e-15))] and stock_id == 0
    assert ('expr_seed', 0) in ctx.calls
    assert not getattr(ctx, 'baths', []) and not getattr(ctx, 'exprs', [])       # nothing of the op-by-op program is registered
    assert context._engine.time == pytest.approx(0.01, rel=1e-12)
    integrator.step(3)
    assert len(ctx.runs) == 3 and ctx.runs[2][1] == 3 and len(ctx.stocks) == 1                # no second definition


EXPECTED_OFF = {
    'verlet': ['SAVE_REF', 'EVAL', 'KICK', 'COPY', 'MOVE', 'CONSTRAIN_X', 'EXPR'],
    'middle': ['SAVE_REF', 'EVAL', 'KICK', 'CONSTRAIN_V', 'MOVE', 'BATH', 'MOVE', 'COPY', 'CONSTRAIN_X', 'EXPR'],
    'langevin': ['SAVE_REF', 'EVAL', 'EXPR', 'COPY', 'MOVE', 'CONSTRAIN_X', 'EXPR'],
    'brownian': ['SAVE_REF', 'COPY', 'EVAL', 'EXPR', 'CONSTRAIN_X', 'EXPR'],
}


@pytest.mark.parametrize('kind', ['verlet', 'middle', 'langevin', 'brownian'])
def test_op_by_op_step(recorder, kind):
    integrator = make(kind)
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    context._engine.set_stock_native(False)
    ctx = recorder[-1]
    integrator.step(4)
    assert [run[1] for run in ctx.runs] == [1, 3]
    assert names(ctx.runs[0]) == names(ctx.runs[1]) == EXPECTED_OFF[kind]
    assert ctx.stocks == []
    ops = ctx.runs[1][0]
    dt = 0.002
    by_name = list(zip(names(ctx.runs[1]), ops))
    # which expressions draw random numbers (the library gives only those a counter of the random stream: csrc/run_ops.hip)
    exprs = [op for name, op in by_name if name == 'EXPR']
    random = [any(code & 0xFF == 4 for code in ctx.exprs[op[1]][0]) for op in exprs]        # X_GAUSS = 4
    assert random == dict(verlet=[False], middle=[False], langevin=[True, False], brownian=[True, False])[kind]
    if kind == 'middle':
        assert [op[4] for name, op in by_name if name == 'MOVE'] == [pytest.approx(0.5 * dt, rel=1e-15)] * 2
        assert ctx.baths == [(pytest.approx(math.exp(-dt), rel=1e-15), pytest.approx(KB * 300.0, rel=1e-15))]
    if kind in ('verlet', 'middle'):
        assert [op[4] for name, op in by_name if name == 'KICK'] == [pytest.approx(dt, rel=1e-15)]


def test_without_constraints_and_without_the_op(recorder):
    integrator = make('middle')
    context = openmm.Context(waters(constrained=False), integrator)
    context.setPositions(np.zeros((12, 3)))
    integrator.step(2)
    assert names(recorder[-1].runs[-1]) == ['EVAL', 'STOCK']
    context._engine.set_stock_native(False)
    integrator.step(2)
    assert names(recorder[-1].runs[-1]) == ['EVAL', 'KICK', 'MOVE', 'BATH', 'MOVE', 'COPY', 'EXPR'] and recorder[-1].runs[-1][1] == 2
    # a library without amm_stock_define: the op-by-op step, whatever the switch says
    recorder[0].cls = OldLibrary
    integrator = make('verlet')
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    assert context._engine.stock_native
    integrator.step(1)
    assert names(recorder[-1].runs[0]) == EXPECTED_OFF['verlet']


def test_setters_invalidate_the_program(recorder):
    integrator = make('middle')
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    ctx = recorder[-1]
    integrator.step(1)
    integrator.setTemperature(350 * unit.kelvin)
    integrator.step(1)
    integrator.setFriction(3 / unit.picosecond)
    integrator.step(1)
    integrator.setStepSize(1 * unit.femtoseconds)
    integrator.step(1)
    assert [(s[1], s[2], s[3]) for s in ctx.stocks] == [
        (pytest.approx(0.002), 1.0, pytest.approx(KB * 300.0)), (pytest.approx(0.002), 1.0, pytest.approx(KB * 350.0)),
        (pytest.approx(0.002), 3.0, pytest.approx(KB * 350.0)), (pytest.approx(0.001), 3.0, pytest.approx(KB * 350.0))]
    assert [run[0][-1][1] for run in ctx.runs] == [0, 1, 2, 3]          # each run's STOCK op names the new definition
    assert context._engine.time == pytest.approx(0.007, rel=1e-12)
    integrator.setRandomNumberSeed(11)
    integrator.step(1)
    assert ('expr_seed', 11) in ctx.calls
    assert ctx.constraints == (12, 1e-5)
    integrator.setConstraintTolerance(1e-9)
    assert ctx.constraints == (12, 1e-9) and integrator.getConstraintTolerance() == 1e-9
    assert ('constraints_set_tolerance', 1e-9) in ctx.calls             # the set is kept, its tolerance changed
    integrator.step(1)
    assert names(ctx.runs[-1]) == ['EVAL', 'STOCK']
    context._engine.set_stock_native(False)
    integrator.step(1)
    assert names(ctx.runs[-1]) == EXPECTED_OFF['middle']


def test_several_ranks_are_refused(recorder, monkeypatch):
    class World:
        world = 2

        def barrier(self, rank):
            pass
    monkeypatch.setattr(E.LocalWorld, 'current', staticmethod(lambda: (World(), 0)))
    for kind in ('middle', 'langevin', 'brownian'):
        with pytest.raises(NotImplementedError, match='stock integrators run on one rank'):
            openmm.Context(waters(), make(kind))
    # a VerletIntegrator could always be bound on several ranks (static energies, minimisations): it is refused when it steps
    integrator = make('verlet')
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    with pytest.raises(NotImplementedError, match='stock integrators run on one rank'):
        integrator.step(1)
    assert recorder[-1].runs == []


def test_a_barostat_is_accepted(recorder):
    for kind in ('verlet', 'middle', 'langevin', 'brownian'):
        system = waters()
        barostat = openmm.MonteCarloBarostat(1 * unit.bar, 300 * unit.kelvin, 3)
        barostat.setRandomNumberSeed(5)
        system.addForce(barostat)
        integrator = make(kind)
        context = openmm.Context(system, integrator)
        context.setPositions(np.random.default_rng(2).uniform(0, 3, (12, 3)))
        ctx = recorder[-1]
        integrator.step(7)
        # the attempt precedes every third step: 2 steps (the first on its own), 3 and 2, with an attempt in front of the 3 and the 2
        assert [run[1] for run in ctx.runs] == [1, 1, 3, 2]
        assert [c[0] for c in ctx.calls if c[0] == 'mol_scale'] == ['mol_scale'] * 2
        assert all(names(run) == ['EVAL', 'STOCK'] for run in ctx.runs)
        assert context._engine.barostat_stats['attempts'] == 2


def test_free_space_system(recorder):
    system = waters(box=False)
    nb = openmm.NonbondedForce()
    nb.setNonbondedMethod(openmm.NonbondedForce.NoCutoff)
    for k in range(12):
        nb.addParticle(0.0, 0.3, 0.5)
    system.addForce(nb)
    integrator = make('middle')
    context = openmm.Context(system, integrator)
    assert context._engine.free_space
    context.setPositions(np.random.default_rng(2).uniform(0, 3, (12, 3)))
    integrator.step(2)
    assert names(recorder[-1].runs[0]) == ['EVAL', 'STOCK']


def test_verlet_with_step_size_zero_still_serves_static_energies(recorder):
    """VerletIntegrator(0.0) as the reference's static energy checks use it: nothing is compiled or run, a State comes back."""
    integrator = openmm.VerletIntegrator(0.0)
    context = openmm.Context(waters(), integrator)
    context.setPositions(np.zeros((12, 3)))
    ctx = recorder[-1]
    state = context.getState(getEnergy=True, getForces=True, getPositions=True)
    assert state.getPotentialEnergy()._value == 0.0 and state.getKineticEnergy()._value == 0.0
    assert ctx.runs == [] and ctx.stocks == [] and not getattr(ctx, 'exprs', [])
    assert [c for c in ctx.calls if c[0] == 'force_eval']
    assert context.getIntegrator() is integrator and integrator.getStepSize()._value == 0.0
    assert context._engine.time == 0.0

