"""CPU tests of the regulated propagators (propagators.py:1537-2117 of the reference): the emitted program text against the
reference's captures (tests/golden/regulated_programs.json, scripts/capture_reference_text.py), and the ops the engine compiles
them to -- recorded by a context that stands in for the HIP library (no GPU)."""
import json
import math
import os

import pytest

import atomsmm_amd as atomsmm
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.testing import system_from_arrays
from atomsmm_amd.utils import kB
from fake_backend import RecordingContext

T, TAU, GAMMA = 300 * unit.kelvin, 10 * unit.femtoseconds, 10 / unit.picoseconds
BATHS = {3: atomsmm.RegulatedMassiveNoseHooverLangevinPropagator, 4: atomsmm.TwiceRegulatedMassiveNoseHooverLangevinPropagator,
         5: atomsmm.RegulatedAtomicNoseHooverLangevinPropagator, 6: atomsmm.TwiceRegulatedAtomicNoseHooverLangevinPropagator}


def _captured():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'regulated_programs.json')) as fh:
        return json.load(fh)['programs']


@pytest.mark.parametrize('name', sorted(_captured()))
def test_regulated_program_equals_the_reference_capture(name):
    g = _captured()[name]
    integ = eval(g['ctor'], {'atomsmm': atomsmm, 'unit': unit})
    assert [integ.getPerDofVariableName(i) for i in range(integ.getNumPerDofVariables())] == g['per_dof']
    names = [integ.getGlobalVariableName(i) for i in range(integ.getNumGlobalVariables())]
    assert names == g['globals']
    for i, gname in enumerate(names):
        assert integ.getGlobalVariable(i) == pytest.approx(g['global_values'][gname], rel=1e-9, abs=1e-300), gname
    assert integ.pretty_steps() == g['steps']
    assert integ._kinetic == g['kinetic']
    if g['kinetic'] is not None:
        assert integ.getKineticEnergyExpression() == g['kinetic']


def test_unit_sqrt_and_kinetic_expression_default():
    q = unit.sqrt(4 * unit.femtoseconds ** 2)
    assert q._md() == pytest.approx(0.002)
    assert unit.sqrt(9.0) == 3.0
    assert openmm.CustomIntegrator(0.001).getKineticEnergyExpression() == 'm*v*v/2'


class RegulatedRecorder(RecordingContext):
    """The recorder with the regulated entry points of the library (amm_regulated_define, amm_bath_define_regulated)."""

    def regulated_define(self, on, alpha=1.0, an_kT=0.0):
        self.calls.append(('regulated_define', bool(on), alpha, an_kT))

    def bath_define_regulated(self, kind, split, h, z, kT, Q, omega, friction, alpha, an, slot_v_eta):
        self.baths = getattr(self, 'baths', [])
        self.baths.append(dict(kind=kind, split=split, h=h, z=z, kT=kT, Q=Q, omega=omega, friction=friction, alpha=alpha, an=an,
                               slot=slot_v_eta))
        return len(self.baths) - 1


@pytest.fixture
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(RegulatedRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def regulated_context(spcfw, recorder, bath, n=2, alpha=1, move=None, scheme='middle'):
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 7 * unit.angstroms, 5 * unit.angstroms)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    f = atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb)
    f.setForceGroup(2)
    f.addTo(respa)
    move = move or atomsmm.RegulatedTranslationPropagator(T, n, alpha_n=alpha)
    integ = atomsmm.MultipleTimeScaleIntegrator(4 * unit.femtoseconds, [4, 2, 1], move=move,
                                                boost=atomsmm.RegulatedBoostPropagator(), bath=bath, scheme=scheme)
    sim = app.Simulation(app.Topology(), respa, integ, openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(spcfw['positions'] * unit.nanometers)
    return sim, recorder[-1]


def _mode(rec):
    return [c for c in rec.calls if c[0] == 'regulated_define'][-1]


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('kind', sorted(BATHS))
def test_native_composition_ops(spcfw, recorder, kind, split):
    """Each regulated bath in the innermost loop: only KICK / MOVE / EVAL / BATH ops (plus the copies RESPA needs), the context in
    regulated mode with the move's alpha and alpha n kT, and one bath whose constants are the ones the text implies."""
    n, alpha = 3, 2
    sim, rec = regulated_context(spcfw, recorder, BATHS[kind](T, n, TAU, GAMMA, alpha_n=alpha, split=split), n=n, alpha=alpha)
    sim.step(2)
    assert sim.context._engine._interpreted is False
    ops = rec.runs[-1][0]
    assert {o[0] for o in ops} <= {B.OP_KICK, B.OP_MOVE, B.OP_EVAL, B.OP_BATH, B.OP_COPY}
    assert sum(o[0] == B.OP_BATH for o in ops) == 8 and sum(o[0] == B.OP_MOVE for o in ops) == 16
    kT = (kB * T)._md()
    assert _mode(rec) == ('regulated_define', True, alpha, pytest.approx(alpha * n * kT, rel=1e-15))
    assert len(rec.baths) == 1
    b = rec.baths[0]
    tau = TAU._md()
    Q = (3 if kind >= 5 else 1) * kT * tau ** 2
    assert b['kind'] == kind and b['split'] == split and b['alpha'] == alpha and b['an'] == alpha * n
    assert b['h'] == pytest.approx(0.0625 * 0.004, rel=1e-15) and b['z'] == pytest.approx(math.exp(-10.0 * 0.125 * 0.004), rel=1e-15)
    assert b['kT'] == pytest.approx(kT, rel=1e-15) and b['Q'] == pytest.approx(Q, rel=1e-12) and b['friction'] == pytest.approx(10.0)
    assert b['omega'] == pytest.approx(1 / tau if kind < 5 else math.sqrt(kT / Q), rel=1e-12)
    moves = [o for o in ops if o[0] == B.OP_MOVE]
    assert moves[0][4] == pytest.approx(0.0625 * 0.004, rel=1e-15)
    kicks = [o for o in ops if o[0] == B.OP_KICK]
    assert kicks[-1][4] == pytest.approx(0.5 * 0.004, rel=1e-15)


def test_xo_respa_scheme_is_native(spcfw, recorder):
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA)
    sim, rec = regulated_context(spcfw, recorder, bath, scheme='xo-respa')
    sim.step(1)
    ops = rec.runs[-1][0]
    assert {o[0] for o in ops} <= {B.OP_KICK, B.OP_MOVE, B.OP_EVAL, B.OP_BATH, B.OP_COPY}
    assert sum(o[0] == B.OP_BATH for o in ops) == 2 and _mode(rec)[1] is True


def test_adiabatic_bath_takes_the_general_path(spcfw, recorder):
    """Per-DOF kT: neither the moves nor the bath are native -- per-DOF expressions (EXPR ops), and the mode stays off."""
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA, adiabatic=True)
    sim, rec = regulated_context(spcfw, recorder, bath)
    sim.context._engine.fill_per_dof('kT', (kB * T)._md())
    sim.step(1)
    ops = rec.runs[-1][0]
    assert B.OP_EXPR in {o[0] for o in ops} and not getattr(rec, 'baths', [])
    assert not [o for o in ops if o[0] == B.OP_MOVE]
    assert _mode(rec)[1] is False


def test_plain_and_regulated_moves_take_the_general_path(spcfw, recorder):
    """A regulated bath with plain moves is native; a program that mixes plain and regulated moves runs the regulated ones as
    expressions, with the mode off."""
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA)
    move = atomsmm.ChainedPropagator([atomsmm.TranslationPropagator(constrained=False),
                                      atomsmm.RegulatedTranslationPropagator(T, 2)])
    sim, rec = regulated_context(spcfw, recorder, bath, move=move)
    sim.step(1)
    ops = rec.runs[-1][0]
    assert B.OP_EXPR in {o[0] for o in ops} and B.OP_MOVE in {o[0] for o in ops}
    assert _mode(rec)[1] is False


def test_global_variant_runs_on_the_host_walked_path(spcfw, recorder):
    bath = atomsmm.TwiceRegulatedGlobalNoseHooverLangevinPropagator(3 * 1536, T, 2, TAU, GAMMA)
    sim, rec = regulated_context(spcfw, recorder, bath)
    sim.step(1)
    assert sim.context._engine._interpreted is True
    assert _mode(rec)[1] is False
    assert any(c[0] == 'expr_eval' and c[6] for c in rec.calls)          # the ComputeSum of sum_mvv


def test_vector_functions_outside_the_native_bath_are_refused(spcfw, recorder):
    """The atomic baths use dot() and _x(), which the expression interpreter lacks: a block the recogniser does not take (here: a
    drive with one more definition than the reference writes) is refused with NotImplementedError, not run as something else."""
    class Odd(atomsmm.RegulatedAtomicNoseHooverLangevinPropagator):
        def _drive(self):
            return super()._drive() + '; Q=Q'
    sim, rec = regulated_context(spcfw, recorder, Odd(T, 2, TAU, GAMMA))
    with pytest.raises(NotImplementedError, match='vector functions'):
        sim.step(1)


def test_several_ranks_are_refused_at_context_creation(spcfw, recorder):
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA)

    def job(rank):
        with pytest.raises(NotImplementedError, match='one rank'):
            regulated_context(spcfw, recorder, bath)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
