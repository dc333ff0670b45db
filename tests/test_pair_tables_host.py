"""CPU tests of the tabulated functions of a CustomNonbondedForce: the object model (openmm.Continuous1DFunction, Discrete1DFunction,
Discrete2DFunction, addTabulatedFunction), the compiler's table words (expr.compile_pair with `functions`), the host's spline solve
(atomsmm_amd/tables.py) against scipy, and the translation on tests/fake_backend.py -- the calls it records and the errors it raises."""
import copy

import numpy as np
import pytest

import atomsmm_amd as atomsmm
import pair_table_cases as C
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm
from atomsmm_amd import tables as T
from atomsmm_amd.forces import describe_energy
from fake_backend import RecordingContext


# ------------------------------------------------------------------------------------ 1. the object model
def test_function_round_trips():
    u = openmm.Continuous1DFunction([1.0, 2.0, 4.0], 0.2, 0.8)
    assert u.getFunctionParameters() == ([1.0, 2.0, 4.0], 0.2, 0.8)
    u.setFunctionParameters([3.0, 1.0], 0.1, 0.5)
    assert u.getFunctionParameters() == ([3.0, 1.0], 0.1, 0.5)
    f = openmm.Discrete1DFunction([0.5, 1.5, 2.5])
    assert f.getFunctionParameters() == [0.5, 1.5, 2.5]
    f.setFunctionParameters([7.0])
    assert f.getFunctionParameters() == [7.0]
    g = openmm.Discrete2DFunction(2, 3, [0, 1, 2, 3, 4, 5])
    assert g.getFunctionParameters() == (2, 3, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    g.setFunctionParameters(3, 1, [9, 8, 7])
    assert g.getFunctionParameters() == (3, 1, [9.0, 8.0, 7.0])
    for fn in (u, f, g):
        assert isinstance(fn, openmm.TabulatedFunction)


def test_force_keeps_names_indices_and_copies():
    force = openmm.CustomNonbondedForce('A(t1,t2)*U(r)')
    force.addPerParticleParameter('t')
    assert force.getNumTabulatedFunctions() == 0
    u = openmm.Continuous1DFunction([1.0, 2.0, 4.0], 0.2, 0.8)
    a = openmm.Discrete2DFunction(2, 2, [1, 2, 2, 3])
    assert force.addTabulatedFunction('U', u) == 0 and force.addTabulatedFunction('A', a) == 1
    assert force.getNumTabulatedFunctions() == 2
    assert [force.getTabulatedFunctionName(k) for k in range(2)] == ['U', 'A']
    assert force.getTabulatedFunction(0) is u and force.getTabulatedFunction(1) is a          # the object itself: set + update reaches it
    with pytest.raises(openmm.OpenMMException, match='not a TabulatedFunction'):
        force.addTabulatedFunction('V', [1.0, 2.0])
    # deep copies carry the functions (what hijackForce and RESPASystem._copy_from make)
    system = openmm.System()
    system.addParticle(1.0)
    force.addParticle([0])
    system.addForce(force)
    clone = atomsmm.hijackForce(copy.deepcopy(system), 0)
    assert clone is not force and clone.getNumTabulatedFunctions() == 2 and clone.getTabulatedFunctionName(1) == 'A'
    assert clone.getTabulatedFunction(0) is not u and clone.getTabulatedFunction(0).getFunctionParameters() == u.getFunctionParameters()
    assert clone.getTabulatedFunction(1).getFunctionParameters() == a.getFunctionParameters()
    other = openmm.System()
    other._copy_from(system)
    assert other.getForce(0).getTabulatedFunction(1).getFunctionParameters() == (2, 2, [1.0, 2.0, 2.0, 3.0])


def test_constructor_errors_are_openmm_exceptions():
    with pytest.raises(openmm.OpenMMException, match='at least two points'):
        openmm.Continuous1DFunction([1.0], 0.0, 1.0)
    for lo, hi in ((0.5, 0.5), (0.6, 0.5)):
        with pytest.raises(openmm.OpenMMException, match='max <= min'):
            openmm.Continuous1DFunction([1.0, 2.0], lo, hi)
    with pytest.raises(openmm.OpenMMException, match='incorrect number of values'):
        openmm.Discrete2DFunction(2, 3, [1.0] * 5)
    good = openmm.Discrete2DFunction(2, 2, [1.0] * 4)
    with pytest.raises(openmm.OpenMMException, match='incorrect number of values'):
        good.setFunctionParameters(2, 2, [1.0] * 3)
    assert good.getFunctionParameters() == (2, 2, [1.0] * 4)          # a refused set leaves the function as it was


def test_four_refusals_by_name():
    with pytest.raises(NotImplementedError, match=r'Continuous1DFunction\(periodic=True\)'):
        openmm.Continuous1DFunction([1.0, 2.0, 1.0], 0.0, 1.0, True)
    with pytest.raises(NotImplementedError, match='Continuous2DFunction'):
        openmm.Continuous2DFunction(2, 2, [1.0] * 4, 0, 1, 0, 1)
    with pytest.raises(NotImplementedError, match='Continuous3DFunction'):
        openmm.Continuous3DFunction(2, 2, 2, [1.0] * 8, 0, 1, 0, 1, 0, 1)
    with pytest.raises(NotImplementedError, match='Discrete3DFunction'):
        openmm.Discrete3DFunction(2, 2, 2, [1.0] * 8)


# ------------------------------------------------------------------------------------ 2. the compiler
NAMES = {v: k for k, v in X.ALL_OPCODES.items()}
FUNCTIONS = {'U': ('Continuous1D', 1), 'f': ('Discrete1D', 1), 'A': ('Discrete2D', 2)}


def words(prog):
    return [(NAMES[w & 0xff], w >> 8) for w in prog.code]


def test_table_words_follow_their_arguments():
    prog = X.compile_pair('A(t1,t2)*U(r) + f(t1)*f(t2)', ['t'], [], FUNCTIONS)
    assert words(prog) == [('PAIR_P1', 0), ('PAIR_P2', 0), ('TAB_D2', 2), ('PAIR_R', 0), ('TAB_C1', 0), ('MUL', 0),
                           ('PAIR_P1', 0), ('TAB_D1', 1), ('PAIR_P2', 0), ('TAB_D1', 1), ('MUL', 0), ('ADD', 0)]
    assert X.table_words(prog.code) == [('TAB_D2', 2), ('TAB_C1', 0), ('TAB_D1', 1), ('TAB_D1', 1)]
    # arguments are expressions like any other, definitions included
    prog = X.compile_pair('U(s*r); s = 0.5*(t1+t2)', ['t'], [], FUNCTIONS)
    assert words(prog)[-2:] == [('MUL', 0), ('TAB_C1', 0)]
    # a text without calls compiles to what it compiled to without `functions`
    plain = 't1*t2*exp(-r)'
    assert X.compile_pair(plain, ['t'], [], FUNCTIONS).code == X.compile_pair(plain, ['t'], []).code
    assert X.table_words(X.compile_pair(plain, ['t'], []).code) == []


def test_opcode_tables():
    assert (X.TABLE_OPCODES['TAB_C1'], X.TABLE_OPCODES['TAB_D1'], X.TABLE_OPCODES['TAB_D2']) == (55, 56, 57)
    assert len(X.PAIR_OPCODES) == 3 and len(X.TABLE_OPCODES) == 3
    others = set(X.OPCODES.values()) | set(X.PAIR_OPCODES.values()) | set(X.TERM_OPCODES.values())
    assert not set(X.TABLE_OPCODES.values()) & others
    assert not set(X.TABLE_OPCODES) & (set(X.OPCODES) | set(X.PAIR_OPCODES) | set(X.TERM_OPCODES))
    assert all(X.ALL_OPCODES[k] == v for k, v in X.TABLE_OPCODES.items())
    assert X.PAIR_MAX_TABLES == 8


def test_arity_shadowing_and_the_table_limit():
    with pytest.raises(X.ExpressionError, match=r'tabulated function U takes 1 argument \(2 given\)'):
        X.compile_pair('U(r, r)', [], [], FUNCTIONS)
    with pytest.raises(X.ExpressionError, match=r'tabulated function A takes 2 arguments \(1 given\)'):
        X.compile_pair('A(t1)*A(t2)', ['t'], [], FUNCTIONS)
    with pytest.raises(X.ExpressionError, match=r'a Discrete2DFunction takes 2 arguments \(1 declared\)'):
        X.compile_pair('r', [], [], {'A': ('Discrete2D', 1)})
    with pytest.raises(X.ExpressionError, match='tabulated function exp shadows the built-in function'):
        X.compile_pair('exp(r)', [], [], {'exp': ('Continuous1D', 1)})
    with pytest.raises(X.ExpressionError, match='tabulated function r shadows the distance r'):
        X.compile_pair('r', [], [], {'r': ('Continuous1D', 1)})
    for name in ('k', 't', 't1'):
        with pytest.raises(X.ExpressionError, match='tabulated function %s shadows the parameter' % name):
            X.compile_pair('k*t1*t2*r', ['t'], ['k'], {name: ('Discrete1D', 1)})
    nine = {'u%d' % k: ('Continuous1D', 1) for k in range(9)}
    with pytest.raises(X.ExpressionError, match=r'at most 8 tabulated functions \(9 given\)'):
        X.compile_pair('u0(r)', [], [], nine)
    nine.pop('u8')
    assert words(X.compile_pair('u7(r)', [], [], nine)) == [('PAIR_R', 0), ('TAB_C1', 7)]
    # the stack walk counts the words: TAB_D2 takes two and leaves one
    deep = 'A(t1, ' * 15 + 't2' + ')' * 15
    X.compile_pair(deep, ['t'], [], FUNCTIONS)
    with pytest.raises(X.ExpressionError, match=r'stack depth 17 \(limit 16\)'):
        X.compile_pair('A(t1, ' * 16 + 't2' + ')' * 16, ['t'], [], FUNCTIONS)
    # the other compilers do not learn the words
    with pytest.raises(X.ExpressionError, match='unsupported function call: U/1'):
        X.compile_term('U(r)', ['r'], [], [])


def test_eval_global_takes_callables():
    assert X.eval_global('2*g(x, 3) + h(x)', dict(x=2.0), functions=dict(g=lambda a, b: a * b, h=lambda a: -a)) == 10.0
    with pytest.raises(X.ExpressionError, match='unsupported'):
        X.eval_global('g(x)', dict(x=2.0))


# ------------------------------------------------------------------------------------ 3. the host's spline against scipy
def _values(knots, lo, hi):
    r = np.linspace(lo, hi, knots)
    return 3.0 + 0.5 * np.sin(2.0 * r)


@pytest.mark.parametrize('knots', [5, 6, 901])
def test_host_spline_against_scipy(knots):
    """Value AND derivative at the knots, at the midpoints, and at points of the first and the last interval: within 1e-13 of the
    largest |value|.  The function is chosen for what that bound can resolve in a derivative: the reference rounds its knots
    (linspace) and divides by their differences, which puts (knots - 1) * 1.1e-16 * |S'| = 1e-13 |S'| into its own slope at 901 knots
    -- so |S'| <= 1 under |S| <= 3.5 leaves a factor of three.  (The tabulated U of the GPU tests, |S'| = 30 |S|, agrees with scipy
    to 4e-16 max |S| and 3e-14 max |S'|, 9e-13 max |S|: tests/test_gpu_pair_tables.py compares sums over it at 1e-10 and 1e-9.)"""
    lo, hi = 0.14, 1.0
    y = _values(knots, lo, hi)
    coef = T.spline_coefficients(y, lo, hi)
    assert coef.shape == (knots - 1, 4)
    s_ref, d_ref = C.reference_spline(y, lo, hi)
    x = np.linspace(lo, hi, knots)
    h = x[1] - x[0]
    points = np.concatenate([x, 0.5 * (x[:-1] + x[1:]), lo + h * np.array([1e-9, 0.1, 0.37, 0.9, 1 - 1e-9]),
                             hi - h * np.array([1 - 1e-9, 0.9, 0.37, 0.1, 1e-9])])
    value, slope = T.spline_eval(coef, lo, hi, points)
    ev, ed = np.abs(value - s_ref(points)).max(), np.abs(slope - d_ref(points)).max()
    sv = np.abs(s_ref(points)).max()
    print('%d knots: max |dS| = %.2e, max |dS\'| = %.2e of max |S| = %.3g' % (knots, ev / sv, ed / sv, sv))
    assert ev <= 1e-13 * sv
    assert ed <= 1e-13 * sv
    # natural ends, the knots themselves, and nothing outside
    m = T.spline_second_derivatives(y, lo, hi)
    assert m[0] == 0.0 and m[-1] == 0.0 and coef[0, 2] == 0.0
    assert np.array_equal(coef[:, 0], y[:-1])
    out_v, out_d = T.spline_eval(coef, lo, hi, np.array([lo - 1e-12, hi + 1e-12, -5.0, 50.0]))
    assert not out_v.any() and not out_d.any()
    end_v, _ = T.spline_eval(coef, lo, hi, np.array([lo, hi]))
    assert end_v[0] == y[0] and abs(end_v[1] - y[-1]) <= 1e-13 * sv


def test_two_knots_are_a_straight_line():
    coef = T.spline_coefficients([3.0, 1.0], 0.2, 0.6)
    assert coef.shape == (1, 4) and coef[0, 0] == 3.0 and coef[0, 1] == pytest.approx(-5.0, rel=1e-15) and not coef[0, 2:].any()


def test_host_callables_follow_the_nan_rule():
    f = T.host_callable(openmm.Discrete1DFunction([5.0, 6.0, 7.0]))
    g = T.host_callable(openmm.Discrete2DFunction(2, 3, [0, 1, 2, 3, 4, 5]))
    assert (f(0.0), f(1.4), f(2.49)) == (5.0, 6.0, 7.0)
    assert g(1.0, 2.0) == 5.0 and g(0.0, 1.0) == 2.0          # values[i + xsize*j]
    for bad in (f(-0.6), f(2.6), f(float('nan')), g(2.0, 0.0), g(0.0, 3.0), g(0.0, float('nan'))):
        assert bad != bad


# ------------------------------------------------------------------------------------ 4. the translation: recorded calls, errors
class Recorder(RecordingContext):
    def pair_expr_create(self, desc, code, consts, globals_, p0, p1, p2, excl_pairs=None, skin=-1.0):
        fid = self._new()
        self.pairs.append(dict(id=fid, family=desc.family, code=list(code), params=[p0.copy(), p1.copy(), p2.copy()]))
        self.calls.append(('pair_expr_create', fid))
        return fid

    def pair_expr_set_globals(self, fid, globals_):
        self.calls.append(('pair_expr_set_globals', fid, list(globals_)))

    def pair_expr_set_tables(self, fid, tables):
        self.calls.append(('pair_expr_set_tables', fid, [(k, nx, ny, lo, hi, np.array(data)) for k, nx, ny, lo, hi, data in tables]))


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


TEXT = 'A(t1,t2)*exp(-r) + f(t1)*f(t2)*U(r)'
SYMMETRIC = [1.0, 2.0, 2.0, 3.0]


def typed_system(types=(0, 1, 1, 0, 1, 0), matrix=SYMMETRIC, text=TEXT, functions=True):
    system = openmm.System()
    for _ in types:
        system.addParticle(12.0)
    system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    force = openmm.CustomNonbondedForce(text)
    force.addPerParticleParameter('t')
    for t in types:
        force.addParticle([t])
    made = {}
    if functions:
        made = dict(U=openmm.Continuous1DFunction([4.0, 2.0, 1.0, 0.5, 0.25, 0.125], 0.2, 1.0), A=openmm.Discrete2DFunction(2, 2, matrix),
                    f=openmm.Discrete1DFunction([0.5, 1.5]))
        for name in ('U', 'A', 'f'):          # the force's order: U = 0, A = 1, f = 2
            force.addTabulatedFunction(name, made[name])
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.9)
    system.addForce(force)
    return system, force, made


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


def table_calls(rec):
    return [c for c in rec.calls if c[0] == 'pair_expr_set_tables']


def test_tables_are_uploaded_in_force_order_and_again_on_update(recorder):
    system, force, made = typed_system()
    assert describe_energy(force.getEnergyFunction(), {}) is None
    context = context_of(system)
    rec = recorder[-1]
    (entry,) = context._engine.entries
    assert X.table_words(entry.program.code) == [('TAB_D2', 1), ('TAB_D1', 2), ('TAB_D1', 2), ('TAB_C1', 0)]
    (call,) = table_calls(rec)
    assert rec.calls.index(call) > rec.calls.index(('pair_expr_create', call[1]))
    u, a, f = call[2]
    assert u[:5] == (T.CONTINUOUS1D, 6, 1, 0.2, 1.0) and u[5].shape == (20,) and u[5][0] == 4.0 and u[5][4] == 2.0
    assert a[:3] == (T.DISCRETE2D, 2, 2) and list(a[5]) == SYMMETRIC
    assert f[:3] == (T.DISCRETE1D, 2, 1) and list(f[5]) == [0.5, 1.5]
    # setFunctionParameters + updateParametersInContext: the tables again, and the per-particle values
    made['A'].setFunctionParameters(2, 2, [1.0, 5.0, 5.0, 3.0])
    force.setParticleParameters(0, [1])
    force.updateParametersInContext(context)
    first, second = table_calls(rec)
    assert list(second[2][1][5]) == [1.0, 5.0, 5.0, 3.0] and second[1] == first[1]
    assert [c for c in rec.calls if c[0] == 'pair_set_params'][-1][2][0] == 1.0


def test_a_force_without_functions_records_no_table_call(recorder):
    system, force, _ = typed_system(text='t1*t2*exp(-r)', functions=False)
    context = context_of(system)
    force.updateParametersInContext(context)
    assert table_calls(recorder[-1]) == []
    # nor does one whose text calls none of its functions
    system, force, _ = typed_system(text='t1*t2*exp(-r)')
    context = context_of(system)
    force.updateParametersInContext(context)
    assert table_calls(recorder[-1]) == [] and context._engine.entries[0].pair_expr is True


def test_a_function_on_a_recognised_text_is_ignored(recorder):
    import pair_expr_cases as P
    system = openmm.System()
    for _ in range(4):
        system.addParticle(12.0)
    system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    force = openmm.CustomNonbondedForce('S*(4*epsilon*((sigma/r)^12-(sigma/r)^6) + Kc*chargeprod/r); S = 1 + step(r - rs0)*u^3*(15*u - 6*u^2 - 10);'
                                        'u=(r-rs0)/(rc0-rs0); ' + P.MIXING)
    for name in ('charge', 'sigma', 'epsilon'):
        force.addPerParticleParameter(name)
    for name, value in dict(Kc=P.KC, rc0=0.9, rs0=0.7).items():
        force.addGlobalParameter(name, value)
    for k in range(4):
        force.addParticle([0.1 * k, 0.3, 0.5])
    force.addTabulatedFunction('unused', openmm.Discrete1DFunction([1.0]))
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.9)
    system.addForce(force)
    context = context_of(system)
    assert context._engine.entries[0].pair_expr is False and table_calls(recorder[-1]) == []


def test_asymmetric_matrix_is_not_symmetric_in_the_particles(recorder):
    system, _, _ = typed_system(matrix=[1.0, 2.0, 2.5, 3.0])
    with pytest.raises(atomsmm.InputError, match='not symmetric in particles 1 and 2'):
        context_of(system)
    context_of(typed_system()[0])
    # the existing callers' signature: still the uniform draws
    E.Engine.check_pair_symmetry('sigma1*sigma2*r', ['sigma'], {})


def test_fractional_and_out_of_range_types_name_the_particle(recorder):
    with pytest.raises(openmm.OpenMMException, match=r'particle 2 has t = 0.5, passed to the tabulated function A as an index'):
        context_of(typed_system(types=(0, 1, 0.5, 0))[0])
    with pytest.raises(openmm.OpenMMException, match=r'particle 3 has t = 2.0.*whole number in 0 \.\. 1'):
        context_of(typed_system(types=(0, 1, 1, 2))[0])
    with pytest.raises(openmm.OpenMMException, match=r'particle 0 has t = -1.0'):
        context_of(typed_system(types=(-1, 1, 1, 0))[0])
    # ... and at updateParametersInContext
    system, force, _ = typed_system()
    context = context_of(system)
    force.setParticleParameters(4, [3])
    with pytest.raises(openmm.OpenMMException, match='particle 4 has t = 3.0'):
        force.updateParametersInContext(context)
    # an index computed by arithmetic is left to the kernel's NaN rule
    context_of(typed_system(text='A(t1,t2)*exp(-r) + f(t1+t2-t1)*f(t2+t1-t2)*U(r)', types=(0, 1, 1, 0))[0])
