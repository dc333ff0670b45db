"""CPU tests of CustomGBForce: what expr.compile_custom_gb emits for the two test models (tests/custom_gb_cases.py) and every limit
it names, the symmetry check of the pair energy terms, what the engine hands to the library (on the call recorder) and everything it
refuses, and the three builders of atomsmm_amd.customgb against the closed forms of their models."""
import copy
import math

import numpy as np
import pytest

import atomsmm_amd as atomsmm
from atomsmm_amd import backend as B
from atomsmm_amd import customgb
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.testing import system_from_arrays
from fake_backend import RecordingContext
import custom_gb_cases as M
import expr_reference as R
import gb_cases as G

OPS = {v: k for k, v in X.ALL_OPCODES.items()}


def words(prog):
    return [(OPS[w & 0xff], w >> 8) for w in prog.code]


class CgbRecorder(RecordingContext):
    def custom_gb_create(self, n_values, types, programs, globals_, params, excl_pairs=None, rc=0.0):
        fid = self._new()
        self.cgbs = getattr(self, 'cgbs', [])
        self.cgbs.append(dict(id=fid, n_values=n_values, types=list(types), programs=[(list(c), list(k)) for c, k in programs],
                              globals=list(globals_), params=np.array(params), excl=np.array(excl_pairs), rc=rc))
        self.calls.append(('custom_gb_create', fid))
        return fid

    def custom_gb_set_params(self, fid, params):
        self.calls.append(('custom_gb_set_params', fid, np.array(params)))

    def custom_gb_set_globals(self, fid, globals_):
        self.calls.append(('custom_gb_set_globals', fid, list(globals_)))

    def custom_gb_set_tables(self, fid, tables):
        self.calls.append(('custom_gb_set_tables', fid, [(t[0], t[1], t[2], np.array(t[5])) for t in tables]))

    def gb_create(self, *a, **k):
        return self._new()


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(CgbRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


@pytest.fixture(scope='module')
def s33(heaq):
    return full(G.s33(heaq))


def full(raw):
    """The case with everything system_from_arrays reads, plus the radii and scales of gb_cases."""
    return dict(raw, **G.with_radii(raw))


def verlet():
    return openmm.VerletIntegrator(0.001)


def system_with(case, force, method='NoCutoff', **kw):
    system = system_from_arrays(case, nonbondedMethod=method, **kw)
    system.addForce(force)
    return system


# ------------------------------------------------------------------------------------ the compiler
def test_programs_of_obc2_text():
    force = M.obc2_force(G.n5())
    progs = M.compiled(force)
    assert progs.types == [2, 0, 0, 0, 2] and progs.globals_ == ['solventDielectric', 'soluteDielectric']
    assert progs.value_reads == [(), (0,)] and progs.term_reads == [(1,), (1,), (1,)]
    integral, born = (words(p) for p in progs.values)
    # the pair integral reads r, or of particle 1 (parameter 1) and sr of particle 2 (parameter 8 + 2), no value and no global
    assert {w for w in integral if w[0] in ('TERM_VAR', 'TERM_P', 'GLOBAL')} == {('TERM_VAR', 0), ('TERM_P', 1), ('TERM_P', 10)}
    assert ('max', 0) in integral and ('step', 0) in integral and ('log', 0) in integral and ('abs', 0) in integral
    # the Born radius reads or (parameter 1) and I (variable 1 + 0)
    assert {w for w in born if w[0] in ('TERM_VAR', 'TERM_P')} == {('TERM_VAR', 1), ('TERM_P', 1)} and ('tanh', 0) in born
    self_term, surface, pair = (words(p) for p in progs.terms)
    # globals are numbered in the FORCE's order in every program: soluteDielectric is 1, solventDielectric 0
    assert {w for w in self_term if w[0] == 'GLOBAL'} == {('GLOBAL', 0), ('GLOBAL', 1)}
    assert {w for w in self_term if w[0] in ('TERM_VAR', 'TERM_P')} == {('TERM_P', 0), ('TERM_VAR', 2)}
    assert {w for w in surface if w[0] in ('TERM_VAR', 'TERM_P')} == {('TERM_P', 1), ('TERM_VAR', 2)}
    # the pair term: r, q1, q2, B1 (variable 1 + 1) and B2 (variable 5 + 1)
    assert {w for w in pair if w[0] in ('TERM_VAR', 'TERM_P')} == {('TERM_VAR', 0), ('TERM_P', 0), ('TERM_P', 8), ('TERM_VAR', 2), ('TERM_VAR', 6)}
    assert all(p.globals_ == progs.globals_ for p in progs.programs)


def test_programs_of_chain_table():
    progs = M.compiled(M.chain_force(G.n5()))
    assert progs.types == [1, 0, 0, 1, 2, 0] and progs.globals_ == ['kappa', 'eps0']
    assert progs.value_reads == [(), (0,), (0, 1)] and progs.term_reads == [(1, 2), (), (0, 1, 2)]
    value0 = words(progs.values[0])
    # W(t1, t2): both arguments, then the word of table 0; S(r): r, then the word of table 1
    assert value0[:3] == [('TERM_P', 0), ('TERM_P', 8), ('TAB_D2', 0)]
    assert value0[value0.index(('TAB_C1', 1)) - 1] == ('TERM_VAR', 0)
    assert ('GLOBAL', 0) in value0 and ('TERM_P', 9) in value0
    assert X.table_words(progs.values[0].code) == [('TAB_D2', 0), ('TAB_C1', 1)]
    assert ('GLOBAL', 1) in words(progs.values[2]) and ('GLOBAL', 0) in words(progs.terms[1])
    pair = words(progs.terms[0])
    assert {w for w in pair if w[0] == 'TERM_VAR'} == {('TERM_VAR', 0), ('TERM_VAR', 2), ('TERM_VAR', 3), ('TERM_VAR', 6), ('TERM_VAR', 7)}


def test_a_value_sees_only_the_values_before_it():
    with pytest.raises(X.ExpressionError, match='computed value A: unknown symbol in custom-GB expression: B'):
        X.compile_custom_gb(['q'], [], [('A', 'q+B', 0), ('B', 'A*2', 0)], [])
    with pytest.raises(X.ExpressionError, match='computed value V: unknown symbol in custom-GB expression: q'):
        X.compile_custom_gb(['q'], [], [('V', 'q*r', 1)], [])          # a bare parameter in a pair text
    with pytest.raises(X.ExpressionError, match='energy term 0: unknown symbol in custom-GB expression: r'):
        X.compile_custom_gb(['q'], [], [], [('q*r', 0)])              # r in a single-particle text


def test_every_limit_is_named():
    C = X.compile_custom_gb
    with pytest.raises(X.ExpressionError, match='at most 8 per-particle parameters .9 given'):
        C(['p%d' % k for k in range(9)], [], [], [('1', 0)])
    with pytest.raises(X.ExpressionError, match='at most 4 computed values .5 given'):
        C(['q'], [], [('v%d' % k, 'q', 0) for k in range(5)], [])
    with pytest.raises(X.ExpressionError, match='at most 8 energy terms .9 given'):
        C(['q'], [], [], [('q', 0)] * 9)
    with pytest.raises(X.ExpressionError, match='at most 48 global parameters .49 given'):
        C(['q'], ['g%d' % k for k in range(49)], [], [('q', 0)])
    with pytest.raises(X.ExpressionError, match='at most 8 tabulated functions .9 given'):
        C(['q'], [], [], [('q', 0)], {'f%d' % k: ('Discrete1D', 1) for k in range(9)})
    with pytest.raises(X.ExpressionError, match=r'energy term 0: custom-GB expression: 257 code words .limit 256'):
        C(['q'], [], [], [('+'.join(['q'] * 129), 0)])
    with pytest.raises(X.ExpressionError, match=r'energy term 0: custom-GB expression: 49 constants .limit 48'):
        C(['q'], [], [], [('+'.join('q*%d.5' % k for k in range(49)), 0)])
    deep = 'q'
    for k in range(17):
        deep = 'q+(q*(%s))' % deep if k % 2 else 'q*(q+(%s))' % deep
    with pytest.raises(X.ExpressionError, match=r'stack depth \d+ .limit 16'):
        C(['q'], [], [], [(deep, 0)])
    many = 'a0' + ''.join('; a%d = a%d + q' % (k, k + 1) for k in range(17)) + '; a17 = q'
    with pytest.raises(X.ExpressionError, match='more than 16 auxiliary definitions'):
        C(['q'], [], [], [(many, 0)])
    with pytest.raises(X.ExpressionError, match='the computed value B is a sum over pairs in place 1; only the first'):
        C(['q'], [], [('A', 'q', 0), ('B', 'q1*r', 1)], [])
    with pytest.raises(X.ExpressionError, match='unknown computation type 3'):
        C(['q'], [], [('A', 'q', 3)], [])
    with pytest.raises(X.ExpressionError, match='the particle coordinate x in a text is not supported'):
        C(['q'], [], [], [('q*x', 0)])
    with pytest.raises(X.ExpressionError, match='a Discrete2DFunction takes 2 arguments .1 declared'):
        C(['q'], [], [], [('q', 0)], {'f': ('Discrete2D', 1)})
    with pytest.raises(X.ExpressionError, match='kind Continuous2D is not one'):
        C(['q'], [], [], [('q', 0)], {'f': ('Continuous2D', 2)})
    with pytest.raises(X.ExpressionError, match='tabulated function f takes 1 argument .2 given'):
        C(['q'], [], [], [('f(q, q)', 0)], {'f': ('Discrete1D', 1)})


@pytest.mark.parametrize('kw', [dict(params=['q', 'q']), dict(params=['q'], values=[('q', '1', 0)]), dict(params=['q'], globals_=['q']),
                                dict(params=['q'], functions={'q': ('Discrete1D', 1)}), dict(params=['q'], values=[('B', 'q', 0), ('B', 'q', 0)]),
                                dict(params=['q'], globals_=['g'], functions={'g': ('Discrete1D', 1)})])
def test_a_name_used_twice_is_an_error(kw):
    with pytest.raises(X.ExpressionError, match='is used twice among the per-particle parameters, computed values, global'):
        X.compile_custom_gb(kw['params'], kw.get('globals_', []), kw.get('values', []), [('1', 0)], kw.get('functions'))


def test_reserved_names():
    with pytest.raises(X.ExpressionError, match='the name r shadows the distance r'):
        X.compile_custom_gb(['r'], [], [], [('1', 0)])
    with pytest.raises(X.ExpressionError, match='the name exp shadows the built-in function'):
        X.compile_custom_gb(['q'], ['exp'], [], [('1', 0)])


def test_python_keywords_are_names():
    """`or` -- the offset radius of the published texts -- `lambda`, `in`: names of OpenMM, keywords of the host language."""
    prog = X.compile_custom_gb(['or', 'in'], ['lambda'], [], [('or*in+lambda', 0)]).terms[0]
    assert words(prog) == [('TERM_P', 0), ('TERM_P', 1), ('MUL', 0), ('GLOBAL', 0), ('ADD', 0)]


# ------------------------------------------------------------------------------------ symmetry
def test_symmetry_check():
    rows = np.array([[0.5, 1.0], [-0.3, 2.0], [0.8, 0.0]])
    check = E.Engine.check_custom_gb_symmetry
    check('q1*q2/sqrt(r^2+B1*B2)', ['q', 't'], ['I', 'B'], {}, rows)
    check('k*(q1*B2+q2*B1)/r', ['q', 't'], ['I', 'B'], {'k': 2.0}, rows)
    with pytest.raises(atomsmm.InputError, match='pair energy term .q1.B2/r. is not symmetric in particles 1 and 2'):
        check('q1*B2/r', ['q', 't'], ['I', 'B'], {}, rows)
    with pytest.raises(atomsmm.InputError, match='not symmetric'):
        check('q1*q2*I1/r', ['q', 't'], ['I', 'B'], {}, rows)              # symmetric in the parameters, not in the values
    # a table that is not symmetric, read symmetrically and not
    w = {'W': lambda x, y: M.W_VALUES[int(x) + 3 * int(y)]}
    types = np.array([[0.0], [1.0], [2.0]])
    check('(W(t1,t2)+W(t2,t1))/r', ['t'], [], {}, types, functions=w)
    with pytest.raises(atomsmm.InputError, match='not symmetric'):
        check('W(t1,t2)/r', ['t'], [], {}, types, functions=w, samples=12)


def test_an_asymmetric_pair_term_is_refused_by_the_context(s33, recorder):
    force = M.obc2_force(s33)
    force.addEnergyTerm('q1*B2/r', force.ParticlePair)
    with pytest.raises(atomsmm.InputError, match='is not symmetric in particles 1 and 2'):
        openmm.Context(system_with(s33, force), verlet())
    # an asymmetric VALUE is what the model is made of
    openmm.Context(system_with(s33, M.chain_force(s33)), verlet())


# ------------------------------------------------------------------------------------ the translation
def test_translation_calls_in_order(s33, recorder):
    force = M.chain_force(s33, rc=0.9)
    force.setForceGroup(3)
    context = openmm.Context(system_with(s33, force, 'CutoffNonPeriodic', cutoff=1.0), verlet())
    rec = recorder[-1]
    assert context._engine.free_space and rec.box is None
    (made,) = rec.cgbs
    progs = M.compiled(force)
    assert made['n_values'] == 3 and made['types'] == [1, 0, 0, 1, 2, 0] and made['rc'] == 0.9
    assert made['programs'] == [(p.code, p.consts) for p in progs.programs]
    assert made['globals'] == [M.KAPPA, M.EPS0]
    assert made['params'].shape == (3, 33) and np.array_equal(made['params'], M.chain_parameters(s33).T)       # parameter-major
    assert made['excl'].tolist() == [list(p) for p in M.chain_exclusions(33)]
    mine = [c for c in rec.calls if c[0].startswith('custom_gb')]
    assert [c[0] for c in mine] == ['custom_gb_create', 'custom_gb_set_tables']
    kinds = [(t[0], t[1], t[2]) for t in mine[1][2]]
    assert kinds == [(2, 3, 3), (0, M.S_KNOTS, 1)] and mine[1][2][0][3].tolist() == M.W_VALUES
    assert len(mine[1][2][1][3]) == 4 * (M.S_KNOTS - 1)           # the spline's coefficients, four per interval
    (entry,) = [e for e in context._engine.entries if e.force is force]
    assert entry.custom_gb == dict(id=made['id'], n_values=3) and entry.term_ids == [made['id']] and not entry.pair_ids
    assert entry.group == 3 and entry.depends == {'kappa', 'eps0'}
    # getState(groups=...) reaches it as a member of its group
    context.setPositions(s33['positions'])
    context.getState(getForces=True, groups={3})
    assert [c for c in rec.calls if c[0] == 'force_eval'] == [('force_eval', made['id'], True)]
    context.getState(getForces=True, groups={0})
    assert [c for c in rec.calls if c[0] == 'force_eval'].count(('force_eval', made['id'], True)) == 1


def test_globals_and_parameters_follow(s33, recorder):
    force = M.chain_force(s33)
    context = openmm.Context(system_with(s33, force), verlet())
    rec = recorder[-1]
    gid = rec.cgbs[0]['id']
    assert context.getParameter('kappa') == M.KAPPA
    context.setParameter('eps0', 2.5)
    assert [c for c in rec.calls if c[0] == 'custom_gb_set_globals'] == [('custom_gb_set_globals', gid, [M.KAPPA, 2.5])]
    # updateParametersInContext: the parameters and the tables' values again, in that order of upload
    force.setParticleParameters(4, [2.0, 0.75, -0.25])
    force.getTabulatedFunction(0).setFunctionParameters(3, 3, [2.0 * v for v in M.W_VALUES])
    del rec.calls[:]
    force.updateParametersInContext(context)
    assert [c[0] for c in rec.calls if c[0].startswith('custom_gb')] == ['custom_gb_set_tables', 'custom_gb_set_params']
    tables = [c for c in rec.calls if c[0] == 'custom_gb_set_tables'][0][2]
    assert tables[0][3].tolist() == [2.0 * v for v in M.W_VALUES]
    params = [c for c in rec.calls if c[0] == 'custom_gb_set_params'][0][2]
    assert params.shape == (3, 33) and params[:, 4].tolist() == [2.0, 0.75, -0.25] and np.array_equal(params[:, 5], M.chain_parameters(s33)[5])
    # what must not change in a live Context
    for change in (lambda: force.addExclusion(0, 5), lambda: force.addEnergyTerm('c', 0), lambda: force.setComputedValueParameters(1, 'P', 'a', 0),
                   lambda: force.setEnergyTermParameters(2, 'c^2', 0)):
        context = openmm.Context(system_with(s33, force), verlet())
        saved = (list(force._exclusions), [list(t) for t in force._terms], [list(v) for v in force._values])
        change()
        with pytest.raises(openmm.OpenMMException, match='cannot change in a live Context'):
            force.updateParametersInContext(context)
        force._exclusions, force._terms, force._values = saved


def test_free_space_decision(s33, spcfw, recorder):
    # alone in a System: free space
    alone = openmm.System()
    for m in s33['mass']:
        alone.addParticle(float(m))
    alone.addForce(M.obc2_force(s33))
    context = openmm.Context(alone, verlet())
    assert context._engine.free_space and len(recorder[-1].cgbs) == 1 and not recorder[-1].pairs
    # next to a NonbondedForce(NoCutoff) and a GBSAOBCForce
    system = system_with(s33, M.obc2_force(s33))
    assert openmm.Context(system, verlet())._engine.free_space
    # next to a periodic NonbondedForce: refused by name, not as a mixture
    water = full(G.d1527(spcfw))
    system = system_from_arrays(dict(water, box=np.full(3, 4.0)), nonbondedMethod='CutoffPeriodic')
    system.addForce(M.obc2_force(water, rc=1.0))
    with pytest.raises(atomsmm.InputError, match='a CustomGBForce in a System with a box-periodic NonbondedForce'):
        openmm.Context(system, verlet())


def test_a_respa_group_takes_the_plain_path(s33, recorder):
    force = M.obc2_force(s33)
    force.setForceGroup(1)
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(system_with(s33, force), integrator)
    context.setPositions(s33['positions'])
    context.setVelocitiesToTemperature(300 * unit.kelvin, 1)
    integrator.step(1)
    rec = recorder[-1]
    gid = rec.cgbs[0]['id']
    assert rec.groups[1][1] == [gid] and gid not in rec.groups[0][1]
    evals = [op for ops, _ in rec.runs for op in ops if op[0] == B.OP_EVAL]
    assert any(op[1] == 1 for op in evals) and any(op[1] == 0 for op in evals)


# ------------------------------------------------------------------------------------ refusals, by name
def test_engine_refusals(s33, spcfw, recorder):
    # CutoffPeriodic
    force = M.obc2_force(s33)
    force.setNonbondedMethod(force.CutoffPeriodic)
    with pytest.raises(atomsmm.InputError, match='CustomGBForce: CutoffPeriodic is not supported'):
        openmm.Context(system_with(s33, force), verlet())
    # the particle count
    short = dict(s33, charge=s33['charge'][:32], radius=s33['radius'][:32], scale=s33['scale'][:32])
    with pytest.raises(openmm.OpenMMException, match='CustomGBForce must have exactly as many particles as the System'):
        openmm.Context(system_with(s33, M.obc2_force(short)), verlet())
    # a pair-type value behind the first
    force = M.obc2_force(s33)
    force.addComputedValue('J', 'q1*q2/r', force.ParticlePair)
    with pytest.raises(atomsmm.InputError, match='the computed value J is a sum over pairs in place 2'):
        openmm.Context(system_with(s33, force), verlet())
    # x, y, z
    force = M.obc2_force(s33)
    force.addEnergyTerm('q*z', force.SingleParticle)
    with pytest.raises(atomsmm.InputError, match='the particle coordinate z in a text is not supported'):
        openmm.Context(system_with(s33, force), verlet())
    # addEnergyParameterDerivative
    force = M.obc2_force(s33)
    force.addEnergyParameterDerivative('solventDielectric')
    with pytest.raises(NotImplementedError, match=r"CustomGBForce.addEnergyParameterDerivative\('solventDielectric'\) is not supported"):
        openmm.Context(system_with(s33, force), verlet())
    # deriv(energy, .): when the Context is created, and from the engine
    custom = openmm.CustomIntegrator(0.001)
    custom.addGlobalVariable('g', 0.0)
    custom.addComputeGlobal('g', 'deriv(energy, soluteDielectric)')
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, ...\) through a CustomGBForce'):
        openmm.Context(system_with(s33, M.obc2_force(s33)), custom)
    context = openmm.Context(system_with(s33, M.obc2_force(s33)), verlet())
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, soluteDielectric\) through a CustomGBForce'):
        context._engine.energy_derivative('soluteDielectric')
    # the virial computers
    water = full(G.d1527(spcfw))
    system = system_from_arrays(dict(water, box=np.full(3, 4.0)), nonbondedMethod='CutoffPeriodic')
    system.addForce(M.obc2_force(water))
    with pytest.raises(NotImplementedError, match='the virial of a CustomGBForce'):
        atomsmm.ComputingSystem(system)
    with pytest.raises(NotImplementedError, match='the virial of a CustomGBForce'):
        atomsmm.PressureComputer(system, app.Topology(1527), openmm.Platform.getPlatformByName('HIP'))
    # a collective variable of a CustomCVForce
    cv = openmm.CustomCVForce('2*e')
    cv.addCollectiveVariable('e', M.obc2_force(s33))
    with pytest.raises(NotImplementedError, match='CustomCVForce over a CustomGBForce'):
        openmm.Context(system_with(s33, cv), verlet())
    # the table classes
    with pytest.raises(NotImplementedError, match='periodic splines are not evaluated'):
        openmm.Continuous1DFunction([0.0, 1.0, 0.0], 0.0, 1.0, periodic=True)
    with pytest.raises(NotImplementedError, match='Continuous2DFunction: two-dimensional splines are not evaluated'):
        openmm.Continuous2DFunction(2, 2, [0.0] * 4, 0, 1, 0, 1)
    with pytest.raises(openmm.OpenMMException, match='not a TabulatedFunction'):
        openmm.CustomGBForce().addTabulatedFunction('f', [1.0, 2.0])
    # a limit, through the Context
    force = M.obc2_force(s33)
    for k in range(3):
        force.addComputedValue('X%d' % k, 'B', force.SingleParticle)
    with pytest.raises(atomsmm.InputError, match='CustomGBForce: not a model .* at most 4 computed values .5 given'):
        openmm.Context(system_with(s33, force), verlet())
    # more than one rank
    system = system_with(s33, M.obc2_force(s33))

    def job(rank):
        with pytest.raises(atomsmm.InputError, match='a CustomGBForce runs on a single rank'):
            openmm.Context(copy.deepcopy(system), verlet())
        return True
    assert E.LocalWorld(2).run(job) == [True, True]


def test_the_size_limit_is_named(recorder):
    n = 32769
    system = openmm.System()
    for _ in range(n):
        system.addParticle(1.0)
    force = openmm.CustomGBForce()
    force.addPerParticleParameter('q')
    force.addEnergyTerm('q', force.SingleParticle)
    force._particles = [[0.0]] * n
    system.addForce(force)
    with pytest.raises(atomsmm.InputError, match='CustomGBForce .* at most 32768 atoms'):
        openmm.Context(system, verlet())


def test_object_model():
    force = openmm.CustomGBForce()
    assert (force.SingleParticle, force.ParticlePair, force.ParticlePairNoExclusions) == (0, 1, 2)
    assert (force.NoCutoff, force.CutoffNonPeriodic, force.CutoffPeriodic) == (0, 1, 2)
    assert force.addPerParticleParameter('q') == 0 and force.addGlobalParameter('g', 2.0) == 0
    assert force.addParticle([0.5]) == 0 and force.addParticle([1.5 * unit.elementary_charge]) == 1
    assert force.addComputedValue('B', 'q*g', force.SingleParticle) == 0 and force.addEnergyTerm('B', 0) == 0
    assert force.addExclusion(0, 1) == 0
    assert (force.getNumParticles(), force.getNumPerParticleParameters(), force.getNumGlobalParameters(), force.getNumComputedValues(),
            force.getNumEnergyTerms(), force.getNumExclusions(), force.getNumTabulatedFunctions(), force.getNumEnergyParameterDerivatives()) == \
        (2, 1, 1, 1, 1, 1, 0, 0)
    assert force.getParticleParameters(1) == (1.5,) and force.getComputedValueParameters(0) == ['B', 'q*g', 0]
    assert force.getEnergyTermParameters(0) == ['B', 0] and force.getExclusionParticles(0) == [0, 1]
    force.setComputedValueParameters(0, 'B', 'q+g', 0)
    force.setEnergyTermParameters(0, 'B^2', 0)
    force.setExclusionParticles(0, 1, 0)
    force.setParticleParameters(0, [0.25])
    assert force.getComputedValueParameters(0)[1] == 'q+g' and force.getEnergyTermParameters(0)[0] == 'B^2'
    assert not force.usesPeriodicBoundaryConditions()
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.8 * unit.nanometer)
    assert force.usesPeriodicBoundaryConditions() and force.getCutoffDistance()._value == 0.8


# ------------------------------------------------------------------------------------ the builders
ALPHA_BETA_GAMMA = dict(GBSAOBC1Force=(0.8, 0.0, 2.909125), GBSAOBC2Force=(1.0, 0.8, 4.85))


def closed_integrand(r, rho, s):
    """h/2 of the HCT pair integral, from the published formula (no engulfed term)."""
    if not rho < r + s:
        return 0.0
    L, U = max(rho, abs(r - s)), r + s
    return 0.5 * (1 / L - 1 / U + 0.25 * (r - s * s / r) * (1 / U ** 2 - 1 / L ** 2) + 0.5 * math.log(L / U) / r)


@pytest.mark.parametrize('builder', ['GBSAHCTForce', 'GBSAOBC1Force', 'GBSAOBC2Force'])
def test_builder_texts_against_the_closed_forms(builder):
    charge, radius, scale = [0.4, -0.3, 0.1], [0.15, 0.12, 0.19], [0.85, 0.8, 0.72]
    force = getattr(customgb, builder)(charge, radius, scale, soluteDielectric=2.0, solventDielectric=60.0, SA=3.0)
    assert isinstance(force, openmm.CustomGBForce) and force.getNumParticles() == 3
    assert [force.getPerParticleParameterName(k) for k in range(3)] == ['q', 'or', 'sr']
    assert force.getParticleParameters(1) == (-0.3, 0.12 - 0.009, 0.8 * (0.12 - 0.009))
    (iname, itext, itype), (bname, btext, btype) = (force.getComputedValueParameters(k) for k in range(2))
    assert (iname, itype, bname, btype) == ('I', force.ParticlePairNoExclusions, 'B', force.SingleParticle)
    assert [force.getEnergyTermParameters(k)[1] for k in range(3)] == [force.SingleParticle, force.SingleParticle, force.ParticlePairNoExclusions]
    glob = dict(soluteDielectric=2.0, solventDielectric=60.0)
    pre = 138.935456 * (1 / 2.0 - 1 / 60.0)
    points = [(0.31, 0.141, 0.09), (0.05, 0.30, 0.08), (0.2, 0.111, 0.15), (0.02, 0.08, 0.2), (1.7, 0.16, 0.13)]     # (r, or1, sr2)
    for r, rho, s in points:
        got = float(R.evaluate(itext, dict(r=r, or1=rho, sr2=s))[0])
        # (the closed form is summed in doubles from terms up to 1/L = 12.5: a handful of roundings of 2^-53 * 12.5 each)
        assert got == pytest.approx(closed_integrand(r, rho, s), rel=1e-13, abs=2e-14)
    for integral, rho in [(0.0, 0.141), (1.3, 0.111), (4.0, 0.2), (2.2, 0.16)]:
        if builder == 'GBSAHCTForce':
            want = 1 / (1 / rho - integral)
        else:
            a, b, c = ALPHA_BETA_GAMMA[builder]
            psi = integral * rho
            want = 1 / (1 / rho - math.tanh(a * psi - b * psi ** 2 + c * psi ** 3) / (rho + 0.009))
        assert float(R.evaluate(btext, {'I': integral, 'or': rho})[0]) == pytest.approx(want, rel=1e-13)
    self_text, sa_text, pair_text = (force.getEnergyTermParameters(k)[0] for k in range(3))
    for q, born, rho in [(0.4, 0.2, 0.141), (-0.3, 0.15, 0.111)]:
        assert float(R.evaluate(self_text, dict(glob, q=q, B=born))[0]) == pytest.approx(-0.5 * pre * q * q / born, rel=1e-13)
        want = 4 * math.pi * 3.0 * (rho + 0.009 + 0.14) ** 2 * ((rho + 0.009) / born) ** 6
        assert float(R.evaluate(sa_text, {'B': born, 'or': rho})[0]) == pytest.approx(want, rel=1e-13)
    for r, b1, b2 in [(0.31, 0.2, 0.15), (1.2, 0.14, 0.3)]:
        f = math.sqrt(r * r + b1 * b2 * math.exp(-r * r / (4 * b1 * b2)))
        assert float(R.evaluate(pair_text, dict(glob, r=r, q1=0.4, q2=-0.3, B1=b1, B2=b2))[0]) == pytest.approx(pre * 0.12 / f, rel=1e-13)
    # no surface term on request; the engulfed term on request
    assert getattr(customgb, builder)(charge, radius, scale, SA=None).getNumEnergyTerms() == 2
    engulfed = getattr(customgb, builder)(charge, radius, scale, engulfed=True).getComputedValueParameters(0)[1]
    r, rho, s = 0.03, 0.091, 0.291
    assert rho < s - r
    want = closed_integrand(r, rho, s) + 0.5 * 2 * (1 / rho - 1 / max(rho, abs(r - s)))
    assert float(R.evaluate(engulfed, dict(r=r, or1=rho, sr2=s))[0]) == pytest.approx(want, rel=1e-13)


def test_obc2_builder_is_the_reference_of_gbsaobcforce():
    """The builder's model with the engulfed term, restated by gb_cases: energy of N5 through the host evaluation of the texts."""
    case = G.n5()
    force = M.obc2_force(case, rc=1.0)
    ref = M.obc2_reference(case, 1.0)
    par = np.array(force._particles)
    pos = case['positions']
    glob = dict(soluteDielectric=1.0, solventDielectric=78.3)
    itext, btext = force.getComputedValueParameters(0)[1], force.getComputedValueParameters(1)[1]
    n = 5
    dist = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    integral = [sum(X.eval_global(itext, dict(r=dist[i, j], or1=par[i, 1], sr2=par[j, 2])) for j in range(n) if j != i and dist[i, j] < 1.0) for i in range(n)]
    born = [X.eval_global(btext, {'I': integral[i], 'or': par[i, 1]}) for i in range(n)]
    assert np.allclose([integral, born], ref['values'], rtol=1e-13, atol=0)
    terms = [force.getEnergyTermParameters(k)[0] for k in range(3)]
    energy = sum(X.eval_global(t, dict(glob, q=par[i, 0], B=born[i], **{'or': par[i, 1]})) for t in terms[:2] for i in range(n))
    energy += sum(X.eval_global(terms[2], dict(glob, r=dist[i, j], q1=par[i, 0], q2=par[j, 0], B1=born[i], B2=born[j]))
                  for i in range(n) for j in range(i + 1, n) if dist[i, j] < 1.0)
    assert energy == pytest.approx(ref['energy'], rel=1e-13)


def test_chain_table_texts_are_the_reference():
    """The same for the synthetic model, tables included: the texts on the host against the torch restatement."""
    case = G.n5()
    force = M.chain_force(case, rc=1.0)
    ref = M.chain_reference(case, 1.0, want_forces=False)
    fns = {name: __import__('atomsmm_amd.tables', fromlist=['x']).host_callable(fn) for name, fn in force._functions}
    par = M.chain_parameters(case)
    pos = case['positions']
    n = 5
    glob = dict(kappa=M.KAPPA, eps0=M.EPS0)
    dist = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    excluded = {frozenset(p) for p in M.chain_exclusions(n)}
    takes = lambda i, j: i != j and dist[i, j] < 1.0          # noqa: E731
    V = [sum(X.eval_global(M.V_TEXT, dict(glob, r=dist[i, j], t1=par[i, 0], t2=par[j, 0], a2=par[j, 1]), functions=fns)
             for j in range(n) if takes(i, j) and frozenset((i, j)) not in excluded) for i in range(n)]
    P = [X.eval_global(M.P_TEXT, dict(a=par[i, 1], V=V[i])) for i in range(n)]
    Q = [X.eval_global(M.Q_TEXT, dict(glob, P=P[i], V=V[i])) for i in range(n)]
    assert np.allclose([V, P, Q], ref['values'], rtol=1e-13, atol=0)
    energy = sum(X.eval_global(M.SINGLE_TEXT, dict(c=par[i, 2], V=V[i], P=P[i], Q=Q[i])) for i in range(n))
    for i in range(n):
        for j in range(i + 1, n):
            if takes(i, j):
                energy += X.eval_global(M.FAR_TEXT, dict(glob, r=dist[i, j]))
                if frozenset((i, j)) not in excluded:
                    energy += X.eval_global(M.PAIR_TEXT, dict(r=dist[i, j], c1=par[i, 2], c2=par[j, 2], P1=P[i], P2=P[j], Q1=Q[i], Q2=Q[j]))
    assert energy == pytest.approx(ref['energy'], rel=1e-13)


# ------------------------------------------------------------------------------------ the library
def test_library_builds_and_exports_the_new_symbols():
    from atomsmm_amd.build import build_hip
    import ctypes
    library = ctypes.CDLL(build_hip())
    names = ('amm_custom_gb_create', 'amm_custom_gb_set_params', 'amm_custom_gb_set_globals', 'amm_custom_gb_set_tables',
             'amm_custom_gb_values', 'amm_custom_gb_release')
    for name in names:
        assert name in B.EXPORTS and hasattr(library, name)
    for name in ('custom_gb_create', 'custom_gb_set_params', 'custom_gb_set_globals', 'custom_gb_set_tables', 'custom_gb_values',
                 'custom_gb_release'):
        assert callable(getattr(B.HipContext, name))
