"""CPU tests of the generic pair-expression force: the compiler (expr.compile_pair) and the dual-number interpreter -- restated in
plain Python, tests/pair_expr_cases.py -- against the independent 50-digit evaluator of the TEXT (tests/expr_reference.py, derivative by
mpmath.diff), the documented errors, the symmetry check, the translation (on tests/fake_backend.py), and the conditioning of every
reference sum the GPU tests compare against."""
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import expr_reference as R
import pair_expr_cases as P
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm
from atomsmm_amd.forces import describe_energy
from fake_backend import RecordingContext

HOST = R.Budget(4)          # math.* within 4 ulp, x^n by repeated multiplication


# ------------------------------------------------------------------------------------ 1. the compiler against the evaluator
@pytest.mark.parametrize('name', ['buckingham', 'wca', 'gauss-coulomb', 'select', 'pow', 'morse'])
def test_program_matches_the_independent_evaluator(name):
    case = P.TEXTS[name]
    prog = X.compile_pair(case['text'], case['names'], case['globals'])
    rng = np.random.default_rng(sum(map(ord, name)))
    done = replaced = 0
    worst_e = worst_d = 0.0
    while done < 200:
        r = float(rng.uniform(0.15, 1.1))
        p1 = [float(rng.uniform(*case['ranges'][n])) for n in case['names']]
        p2 = [float(rng.uniform(*case['ranges'][n])) for n in case['names']]
        g = {k: float(v * rng.uniform(0.8, 1.2)) for k, v in case['globals'].items()}
        try:
            value, bound, slope = P.exact_point(case['text'], P.env_of(case, r, p1, p2, g), HOST)
        except R.Unstable:
            replaced += 1
            continue
        e, d = P.run_program(prog, r, p1, p2, g)
        assert abs(e - value) <= bound, (r, p1, p2, g, e, float(value))
        worst_e = max(worst_e, float(abs(e - value) / bound) if bound else 0.0)
        if slope == 0:
            assert d == 0.0
        else:
            assert abs(d - slope) <= 1e-9 * abs(slope), (r, p1, p2, g, d, float(slope))
            worst_d = max(worst_d, float(abs(d - slope) / abs(slope)))
        done += 1
    print('%s: %d code words, worst |dE|/bound %.2f, worst relative dE\' %.2e, %d draws replaced' %
          (name, len(prog.code), worst_e, worst_d, replaced))
    assert replaced <= 0.05 * (done + replaced)


def test_mixing_rules_have_zero_derivative_even_at_zero():
    """sqrt(eps1*eps2) at eps = 0 (a water hydrogen): f' = inf, the energy does not depend on r through it."""
    case = P.TEXTS['wca']
    prog = X.compile_pair(case['text'], case['names'], {})
    e, d = P.run_program(prog, 0.3, [0.3, 0.0], [0.32, 0.7], {})
    assert e == 0.0 and d == 0.0


# ------------------------------------------------------------------------------------ 2. definitions, names, limits
def test_definitions_in_any_order_and_a_global_named_lambda():
    forward = X.compile_pair('a*b; a = lambda*r; b = a + q1*q2', ['q'], ['lambda'])
    backward = X.compile_pair('a*b; b = a + q1*q2; a = lambda*r', ['q'], ['lambda'])
    assert forward.globals_ == backward.globals_ == ['lambda']
    for prog in (forward, backward):
        e, d = P.run_program(prog, 0.5, [2.0], [3.0], {'lambda': 0.25})
        assert e == 0.125 * (0.125 + 6.0) and d == pytest.approx(0.25 * 6.125 + 0.125 * 0.25, rel=1e-15)
    opc = {v: k for k, v in X.ALL_OPCODES.items()}
    assert {opc[w & 0xff] for w in forward.code} == {'GLOBAL', 'PAIR_R', 'PAIR_P1', 'PAIR_P2', 'MUL', 'ADD', 'LOAD', 'STORE'}
    # the new words collide with none of the existing ones
    assert not set(X.PAIR_OPCODES.values()) & set(X.OPCODES.values()) and len(set(X.PAIR_OPCODES.values())) == 3


def test_unknown_and_forbidden_symbols():
    with pytest.raises(X.ExpressionError, match='unknown symbol in pair expression: sigma'):
        X.compile_pair('sigma*r', ['q'], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in pair expression: q3'):
        X.compile_pair('q1*q3*r', ['q'], [])
    for per_dof in ('x', 'v', 'f', 'm'):
        with pytest.raises(X.ExpressionError, match='unknown symbol in pair expression: ' + per_dof):
            X.compile_pair('r*' + per_dof, ['q'], [])
    for random in ('gaussian', 'uniform'):
        with pytest.raises(X.ExpressionError, match='random numbers'):
            X.compile_pair('r*' + random, ['q'], [])
    with pytest.raises(X.ExpressionError, match='circular'):
        X.compile_pair('a; a = b*r; b = a', [], [])


def test_limits_are_named():
    deep = 'r' + '+(r' * 16 + ')' * 16          # right-nested: 17 operands wait on the stack
    with pytest.raises(X.ExpressionError, match=r'stack depth 17 \(limit 16\)'):
        X.compile_pair(deep, [], [])
    X.compile_pair('r' + '+(r' * 15 + ')' * 15, [], [])
    with pytest.raises(X.ExpressionError, match=r'code words \(limit 256\)'):
        X.compile_pair('+'.join(['r*r'] * 90), [], [])
    with pytest.raises(X.ExpressionError, match=r'49 constants \(limit 48\)'):
        X.compile_pair('+'.join('%d.5*r' % k for k in range(49)), [], [])
    names = ['g%d' % k for k in range(49)]
    with pytest.raises(X.ExpressionError, match=r'49 global parameters \(limit 48\)'):
        X.compile_pair('r*(' + '+'.join(names) + ')', [], names)
    with pytest.raises(X.ExpressionError, match='more than 16 auxiliary definitions'):
        X.compile_pair('+'.join('d%d' % k for k in range(17)) + ';' + ';'.join('d%d = r*%d' % (k, k + 2) for k in range(17)), [], [])
    with pytest.raises(X.ExpressionError, match='at most 3 per-particle parameters'):
        X.compile_pair('a1*b2*c1*d2*r', ['a', 'b', 'c', 'd'], [])


# ------------------------------------------------------------------------------------ 3. the symmetry check
def test_symmetry_check():
    with pytest.raises(atomsmm.InputError, match='energy expression is not symmetric in particles 1 and 2'):
        E.Engine.check_pair_symmetry('sigma1*r', ['sigma'], {})
    E.Engine.check_pair_symmetry('sigma1*sigma2*r', ['sigma'], {})
    for case in P.TEXTS.values():
        E.Engine.check_pair_symmetry(case['text'], case['names'], case['globals'])


# ------------------------------------------------------------------------------------ 4. the translation and its refusals
class Recorder(RecordingContext):
    def pair_expr_create(self, desc, code, consts, globals_, p0, p1, p2, excl_pairs=None, skin=-1.0):
        fid = self._new()
        self.pairs.append(dict(id=fid, family=desc.family, flags=desc.flags, rc=desc.rc, rswitch=desc.rswitch, sign=desc.sign,
                               code=list(code), consts=list(consts), globals=list(globals_), params=[p0.copy(), p1.copy(), p2.copy()],
                               n_excl=0 if excl_pairs is None else len(excl_pairs)))
        return fid

    def pair_expr_set_globals(self, fid, globals_):
        self.calls.append(('pair_expr_set_globals', fid, list(globals_)))


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def small_system(text=P.TEXTS['buckingham']['text'], names=('A', 'B', 'C'), n=6, method=None, box=True, **globals_):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.0)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    force = openmm.CustomNonbondedForce(text)
    for name in names:
        force.addPerParticleParameter(name)
    for name, value in globals_.items():
        force.addGlobalParameter(name, value)
    for k in range(n):
        force.addParticle([1.0 + k + 10 * s for s in range(len(names))])
    force.addExclusion(0, 1)
    force.setNonbondedMethod(force.CutoffPeriodic if method is None else method)
    force.setCutoffDistance(0.9)
    system.addForce(force)
    return system, force


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


def test_generic_text_takes_the_pair_expression_path(recorder):
    system, force = small_system()
    assert describe_energy(force.getEnergyFunction(), {}) is None
    force.setUseSwitchingFunction(True)
    force.setSwitchingDistance(0.8)
    context = context_of(system)
    (pair,) = recorder[-1].pairs
    assert pair['family'] == B.PAIR_EXPR == 7 and pair['flags'] == B.SWITCH and (pair['rc'], pair['rswitch']) == (0.9, 0.8)
    assert pair['n_excl'] == 1 and pair['sign'] == 1.0
    # raw values, slot by slot
    assert np.array_equal(pair['params'][0], 1.0 + np.arange(6)) and np.array_equal(pair['params'][2], 21.0 + np.arange(6))
    (entry,) = context._engine.entries
    assert entry.pair_expr is True and list(entry.program.code) == pair['code'] and entry.update is None
    assert not any(c[0] == 'pair_share_list' for c in recorder[-1].calls)
    # updateParametersInContext: the raw values again
    force.setParticleParameters(2, [7.0, 8.0, 9.0])
    force.updateParametersInContext(context)
    call = [c for c in recorder[-1].calls if c[0] == 'pair_set_params'][-1]
    assert (call[2][2], call[3][2], call[4][2]) == (7.0, 8.0, 9.0)


def test_two_parameters_leave_the_third_slot_zero_and_globals_follow(recorder):
    case = P.TEXTS['gauss-coulomb']
    system, force = small_system(case['text'], case['names'], **case['globals'])
    context = context_of(system)
    (pair,) = recorder[-1].pairs
    (entry,) = context._engine.entries
    assert not pair['params'][1].any() and not pair['params'][2].any()
    assert pair['globals'] == [case['globals'][g] for g in entry.program.globals_] and entry.depends == {'Kc', 'beta'}
    context.setParameter('beta', 2.0)
    assert recorder[-1].calls[-1] == ('pair_expr_set_globals', pair['id'], [2.0 if g == 'beta' else P.KC for g in entry.program.globals_])
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, beta\) of a CustomNonbondedForce with a generic energy expression'):
        context._engine.energy_derivative('beta')


def test_recognised_texts_keep_their_kernels(recorder):
    system, force = small_system('S*(4*epsilon*((sigma/r)^12-(sigma/r)^6) + Kc*chargeprod/r); S = 1 + step(r - rs0)*u^3*(15*u - 6*u^2 - 10);'
                                 'u=(r-rs0)/(rc0-rs0); ' + P.MIXING, ('charge', 'sigma', 'epsilon'), Kc=P.KC, rc0=0.9, rs0=0.7)
    context = context_of(system)
    assert recorder[-1].pairs[0]['family'] == B.NEAR_NONE and context._engine.entries[0].pair_expr is False


def test_clean_errors(recorder):
    system, force = small_system(names=('A', 'B', 'C', 'D'), text='A1*A2*B1*B2*C1*C2*D1*D2*r')
    with pytest.raises(atomsmm.InputError, match='at most 3 per-particle parameters'):
        context_of(system)
    system, force = small_system()
    force.addInteractionGroup({0, 1}, {2, 3})
    with pytest.raises(NotImplementedError, match='not recognised.*takes no interaction groups'):
        context_of(system)
    system, force = small_system()
    force.setUseLongRangeCorrection(True)
    with pytest.raises(NotImplementedError, match='not recognised.*no long-range correction'):
        context_of(system)
    system, force = small_system(text='k*' + P.TEXTS['buckingham']['text'], k=1.0)
    force.addEnergyParameterDerivative('k')
    with pytest.raises(NotImplementedError, match='addEnergyParameterDerivative'):
        context_of(system)
    for method in (openmm.CustomNonbondedForce.NoCutoff, openmm.CustomNonbondedForce.CutoffNonPeriodic):
        system, force = small_system(method=method, box=False)
        with pytest.raises(NotImplementedError, match='not recognised.*CutoffPeriodic only'):
            context_of(system)
    system, force = small_system(text='A1*r', names=('A',))
    with pytest.raises(atomsmm.InputError, match='not symmetric in particles 1 and 2'):
        context_of(system)
    system, force = small_system(text='A1*A2*r*zeta', names=('A',))
    with pytest.raises(atomsmm.InputError, match='not recognised.*unknown symbol in pair expression: zeta'):
        context_of(system)

    def job(rank):
        with pytest.raises(NotImplementedError, match='not recognised.*runs on a single rank'):
            context_of(small_system()[0])
        return True
    assert E.LocalWorld(2).run(job) == [True, True]


# ------------------------------------------------------------------------------------ 5. the input rule of the GPU references
@pytest.mark.parametrize('fixture,name', P.GPU_CASES)
def test_reference_sums_are_well_conditioned(request, fixture, name):
    """For every (text, fixture) the GPU tests use: the reference sum accumulated in plain fp64 agrees with the same terms
    accumulated in mpmath to rel 1e-12 (energy) and 1e-11 max|F| (forces), and its radial tables agree with mpmath between nodes."""
    data = request.getfixturevalue(fixture)
    case = P.TEXTS[name]
    params = P.typed_parameters(case, np.rint(data['mass']), P.SEED)
    tables = {}
    args = (case, params, data['positions'], data['box'], P.CUTOFF[fixture], data['exc_pairs'])
    e, f = P.pair_sum(*args, tables=tables)
    e_x, f_x = P.pair_sum(*args, tables=tables, exact=True)
    worst = max(max(t.check(6)) for t in tables.values())
    print('%s / %s: E = %.15g (rel %.1e), max|F| = %.6g (max|dF| %.1e of it), %d tables, interpolation %.1e' %
          (fixture, name, e, abs(e - e_x) / abs(e_x), np.abs(f_x).max(), np.abs(f - f_x).max() / np.abs(f_x).max(), len(tables), worst))
    assert abs(e - e_x) <= 1e-12 * abs(e_x)
    assert np.abs(f - f_x).max() <= 1e-11 * np.abs(f_x).max()
    assert worst <= 1e-13         # (of the largest value on the piece of the table that holds the radius)
