"""CPU tests of the general CustomCVForce (any energy text over several collective variables, csrc/cv.hip): the compiler
(expr.compile_cv), the interpreter restated in plain Python with one-hot seeds against 50-digit partial derivatives of the TEXT
(tests/expr_reference.py, mpmath.diff), the translation on a recorder over tests/fake_backend.py, its refusals and its limits."""
import math

import mpmath
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import expr_reference as R
import pair_expr_cases as P
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm, unit
from atomsmm_amd.testing import system_from_arrays
from fake_backend import RecordingContext

HOST = R.Budget(4)
NAMES = {v: k for k, v in X.ALL_OPCODES.items()}
PERIODIC_RESTRAINT = '0.5*K*min(d, 6.283185307179586-d)^2; d=abs(phi-s_phi)'


def words(prog):
    return [(NAMES[w & 0xff], w >> 8) for w in prog.code]


# ------------------------------------------------------------------------------------ 1. the compiler
def test_variables_are_the_cvs_then_the_derivative_parameters():
    prog = X.compile_cv(PERIODIC_RESTRAINT, ['phi'], ['s_phi'], ['K', 's_phi'])
    assert ('TERM_VAR', 0) in words(prog) and ('TERM_VAR', 1) in words(prog) and prog.globals_ == ['K']
    assert not [w for w in words(prog) if w[0] in ('TERM_P', 'PAIR_R', 'PAIR_P1', 'PAIR_P2')]
    # a parameter that is no derivative parameter stays a global
    prog = X.compile_cv('a*cv1 + b*cv2', ['cv1', 'cv2'], ['b'], ['a', 'b'])
    assert words(prog) == [('GLOBAL', 0), ('TERM_VAR', 0), ('MUL', 0), ('TERM_VAR', 2), ('TERM_VAR', 1), ('MUL', 0), ('ADD', 0)]
    with pytest.raises(X.ExpressionError, match='unknown symbol in collective-variable expression: r'):
        X.compile_cv('k*r', ['phi'], [], ['k'])
    with pytest.raises(X.ExpressionError, match='a name is used twice'):
        X.compile_cv('phi', ['phi'], ['phi'], ['phi'])


def test_limits_are_named():
    cvs = ['c%d' % k for k in range(17)]
    with pytest.raises(X.ExpressionError, match=r'collective-variable expression: 17 collective variables \(limit 16\)'):
        X.compile_cv('+'.join(cvs), cvs, [], [])
    X.compile_cv('+'.join(cvs[:16]), cvs[:16], [], [])
    ps = ['p%d' % k for k in range(17)]
    with pytest.raises(X.ExpressionError, match=r'collective-variable expression: 17 energy parameter derivatives \(limit 16\)'):
        X.compile_cv('c0*(' + '+'.join(ps) + ')', ['c0'], ps, ps)
    X.compile_cv('c0*(' + '+'.join(ps[:16]) + ')', ['c0'], ps[:16], ps[:16])
    # 86 products of three words each and 85 additions: 343 words; 64 products: 255
    long_text = '+'.join(['c0*c1'] * 86)
    with pytest.raises(X.ExpressionError, match=r'collective-variable expression: \d+ code words \(limit 256\)'):
        X.compile_cv(long_text, ['c0', 'c1'], [], [])
    assert len(X.compile_cv('+'.join(['c0*c1'] * 64), ['c0', 'c1'], [], []).code) == 255
    exact = 'c0+' + '+'.join(['c0*c1'] * 64)            # 257 words
    with pytest.raises(X.ExpressionError, match=r'collective-variable expression: 257 code words \(limit 256\)'):
        X.compile_cv(exact, ['c0', 'c1'], [], [])
    with pytest.raises(X.ExpressionError, match=r'collective-variable expression: stack depth 17 \(limit 16\)'):
        X.compile_cv('c0' + '+(c0' * 16 + ')' * 16, ['c0'], [], [])


# ------------------------------------------------------------------------------------ 2. the interpreter, one-hot seeds, against mpmath
def run_cv_program(prog, values, gvalues, seed):
    """(E, dE/d values[seed]) of a compile_cv program: the interpreter of csrc/pair_expr_vm.h restated in plain Python
    (pair_expr_cases.run_program) with the leaves of csrc/cv.hip -- TERM_VAR k pushes (values[k], 1 if k == seed else 0), what lane
    `seed` of k_cv_apply does.  The seeded variable takes the place of r, the others ride in the neighbour's parameter slots."""
    code = []
    for word in prog.code:
        op, arg = word & 0xff, word >> 8
        if op == X.ALL_OPCODES['TERM_VAR']:
            word = X.ALL_OPCODES['PAIR_R'] if arg == seed else X.ALL_OPCODES['PAIR_P2'] | arg << 8
        elif op == X.ALL_OPCODES['TERM_P'] or op in X.PAIR_OPCODES.values():
            raise ValueError('not a collective-variable op: %d' % op)
        code.append(word)
    pair = X.Program()
    pair.code, pair.consts, pair.globals_ = code, prog.consts, prog.globals_
    return P.run_program(pair, float(values[seed]), [], list(values), gvalues)


# text, collective variables, derivative parameters, other globals, ranges, kinks (quantities that must stay away from zero)
CASES = {
    'quadratic-coupling': dict(text='0.5*k*(d-s)^2 + 0.5*k2*(a-a0)^2', cvs=['d', 'a'], derivs=['s'], globals=dict(k=1000.0, k2=50.0, a0=1.9),
                               ranges=dict(d=(0.1, 0.5), a=(1.0, 3.0), s=(0.1, 0.5)), kinks=lambda v: []),
    'periodic-restraint': dict(text=PERIODIC_RESTRAINT, cvs=['phi'], derivs=['s_phi'], globals=dict(K=200.0),
                               ranges=dict(phi=(-3.14, 3.14), s_phi=(-3.14, 3.14)),
                               kinks=lambda v: [v['phi'] - v['s_phi'], math.pi - abs(v['phi'] - v['s_phi'])]),
    'cos-exp-product': dict(text='A*cos(phi-psi)*exp(-b*d) + s*d', cvs=['phi', 'psi', 'd'], derivs=['s', 'b'], globals=dict(A=12.0),
                            ranges=dict(phi=(-3.0, 3.0), psi=(-3.0, 3.0), d=(0.1, 1.0), s=(-5.0, 5.0), b=(0.5, 4.0)), kinks=lambda v: []),
    'flat-bottom': dict(text='select(step(d-d0), 0.5*k*(d-d0)^2, 0) + w*step(x-x0)*(x-x0)^2', cvs=['d', 'x'], derivs=['d0'],
                        globals=dict(k=3000.0, w=40.0, x0=1.0), ranges=dict(d=(0.1, 1.0), x=(0.0, 2.0), d0=(0.3, 0.8)),
                        kinks=lambda v: [v['d'] - v['d0'], v['x'] - 1.0]),
    'global-exponent': dict(text='eps*(d/d0)^n + c*theta^m', cvs=['d', 'theta'], derivs=['n', 'c'], globals=dict(eps=2.5, d0=0.3, m=2.5),
                            ranges=dict(d=(0.1, 1.0), theta=(0.5, 3.0), n=(1.5, 6.5), c=(-3.0, 3.0)), kinks=lambda v: []),
}


def reference_partials(text, env, names):
    """(f, its rounding bound as a double evaluation, [df/dname]) of the text at env, 50 digits."""
    main, defs = R.parse(text)
    with mpmath.workdps(R.DIGITS):
        value, bound = R._evaluate_one(main, defs, env, HOST)
        slopes = [mpmath.diff(lambda c, s=s: R._evaluate_one(main, defs, dict(env, **{s: c}), R.NO_ROUNDING)[0], mpmath.mpf(env[s]))
                  for s in names]
    return value, bound, slopes


@pytest.mark.parametrize('name', sorted(CASES))
def test_program_with_one_hot_seeds_matches_the_independent_evaluator(name):
    case = CASES[name]
    variables = case['cvs'] + case['derivs']
    prog = X.compile_cv(case['text'], case['cvs'], case['derivs'], list(case['globals']) + case['derivs'])
    rng = np.random.default_rng(sum(map(ord, name)))
    done = replaced = 0
    worst = 0.0
    while done < 40:
        draw = {s: float(rng.uniform(*case['ranges'][s])) for s in variables}
        if not all(abs(q) > 1e-3 for q in case['kinks'](draw)):
            replaced += 1
            continue
        env = dict(case['globals'], **draw)
        try:
            value, bound, slopes = reference_partials(case['text'], env, variables)
        except R.Unstable:
            replaced += 1
            continue
        scale = max(abs(s) for s in slopes)
        for k, slope in enumerate(slopes):
            e, d = run_cv_program(prog, [draw[s] for s in variables], case['globals'], k)
            assert abs(e - value) <= bound, (draw, e, float(value))
            if scale == 0:
                assert d == 0.0
            else:
                assert abs(d - slope) <= 1e-10 * scale, (draw, variables[k], d, float(slope))
                worst = max(worst, float(abs(d - slope) / scale))
        done += 1
    print('%s: %d code words, worst partial derivative error %.2e of the largest, %d draws replaced' % (name, len(prog.code), worst, replaced))
    assert replaced <= 0.35 * (done + replaced)


# ------------------------------------------------------------------------------------ 3. the translation
class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.terms, self.cvs = [], []

    def term_expr_create(self, kind, code, consts, globals_, idx, params, periodic=False):
        fid = self._new()
        self.terms.append(dict(id=fid, kind=kind, code=list(code), globals=list(globals_), idx=np.array(idx), params=np.array(params)))
        return fid

    def term_expr_set_globals(self, fid, globals_):
        self.calls.append(('term_expr_set_globals', fid, list(globals_)))

    def term_expr_set_params(self, fid, params, n_terms):
        self.calls.append(('term_expr_set_params', fid, np.array(params), n_terms))

    def cv_create(self, inner_ids, n_deriv, code, consts, globals_):
        fid = self._new()
        self.cvs.append(dict(id=fid, inner=list(inner_ids), n_deriv=n_deriv, code=list(code), consts=list(consts), globals=list(globals_)))
        return fid

    def cv_set_globals(self, fid, globals_):
        self.calls.append(('cv_set_globals', fid, list(globals_)))

    def cv_set_variables(self, fid, values):
        self.calls.append(('cv_set_variables', fid, list(values)))

    def cv_values(self, fid, pos, n_cv):
        self.calls.append(('cv_values', fid, n_cv))
        return np.arange(n_cv, dtype=np.float64)

    def cv_energy_derivative(self, fid, pos, out):
        self.calls.append(('cv_energy_derivative', fid, len(out)))
        out += self.torch_arange(len(out))

    @staticmethod
    def torch_arange(n):
        import torch
        return torch.arange(1, n + 1, dtype=torch.float64)


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def bare_system(n=8, box=True):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.0)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    return system


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


def torsion_cv(text='theta'):
    t = openmm.CustomTorsionForce(text)
    t.addTorsion(0, 1, 2, 3)
    return t


def restraint_force():
    cv = openmm.CustomCVForce(PERIODIC_RESTRAINT)
    cv.addCollectiveVariable('phi', torsion_cv())
    cv.addGlobalParameter('K', 200.0)
    cv.addGlobalParameter('s_phi', 0.5)
    cv.addEnergyParameterDerivative('s_phi')
    return cv


def mixed_force():
    """Two collective variables: a harmonic bond set (a hand-written kind) and a generic angle text with a global of its own."""
    bonds = openmm.HarmonicBondForce()
    bonds.addBond(0, 1, 0.1, 1000.0)
    bonds.addBond(1, 2, 0.1, 1000.0)
    bonds.setForceGroup(7)          # (an inner force's group is ignored)
    angle = openmm.CustomAngleForce('0.5*ka*scale*(cos(theta)-c0)^2')
    angle.addGlobalParameter('scale', 1.0)
    angle.addPerAngleParameter('ka')
    angle.addPerAngleParameter('c0')
    angle.addAngle(0, 1, 2, [300.0, -0.3])
    cv = openmm.CustomCVForce('a*cv1^2/(1+cv2) + b*cv2')
    cv.addCollectiveVariable('cv1', bonds)
    cv.addCollectiveVariable('cv2', angle)
    cv.addGlobalParameter('a', 2.0)
    cv.addGlobalParameter('b', 0.5)
    cv.addEnergyParameterDerivative('b')
    return cv


def test_general_path_records_one_cv_create(recorder):
    system = bare_system()
    other = openmm.HarmonicBondForce()
    other.addBond(4, 5, 0.1, 500.0)
    system.addForce(other)
    cv = mixed_force()
    system.addForce(cv)
    context = context_of(system)
    rec = recorder[-1]
    assert len(rec.cvs) == 1
    made = rec.cvs[0]
    prog = X.compile_cv('a*cv1^2/(1+cv2) + b*cv2', ['cv1', 'cv2'], ['b'], ['a', 'b'])
    assert made['code'] == list(prog.code) and made['consts'] == list(prog.consts) and made['globals'] == [2.0] and made['n_deriv'] == 1
    # the inner ids in CV order: the bond-list set of the harmonic bonds, then the term-expression force of the angle text
    inner_sets = [b for b in rec.bonded if b['terms'] == [(B.BOND_HARMONIC, 2, False)]]
    assert len(inner_sets) == 1 and len(rec.terms) == 1 and rec.terms[0]['kind'] == B.TERM_ANGLE
    assert made['inner'] == [inner_sets[0]['id'], rec.terms[0]['id']]
    assert ('cv_set_variables', made['id'], [0.5]) in rec.calls
    entry = [e for e in context._engine.entries if e.force is cv][0]
    assert entry.cv['id'] == made['id'] and entry.cv['names'] == ['cv1', 'cv2'] and entry.cv['derivs'] == ['b']
    assert entry.term_ids == [made['id']] and not entry.term_expr and entry.bonded_id is None and not entry.terms and not entry.pair_ids
    assert entry.depends == {'a', 'b', 'scale'} and list(entry.program.code) == made['code']
    # membership: the object is the last member of its group; the inner forces are in no group
    index, slot, reduced = context._engine._define_group(0)
    members = rec.groups[index][1]
    assert members[-1] == made['id'] and len(members) == 2
    context._engine._define_group('all')
    for _, ids in rec.groups.values():
        assert not set(ids) & set(made['inner'])
    # the energy loops reach it through term_ids, and only it
    context.getState(getEnergy=True)
    evaluated = [c[1] for c in rec.calls if c[0] == 'force_eval']
    assert made['id'] in evaluated and not set(evaluated) & set(made['inner'])
    assert cv.getCollectiveVariableValues(context) == (0.0, 1.0) and rec.calls[-1] == ('cv_values', made['id'], 2)
    assert cv.usesPeriodicBoundaryConditions() is False and cv.getNumEnergyParameterDerivatives() == 1


def test_parameter_changes_reach_the_object_that_reads_them(recorder):
    system = bare_system()
    cv = mixed_force()
    system.addForce(cv)
    context = context_of(system)
    rec = recorder[-1]
    cid, tid = rec.cvs[0]['id'], rec.terms[0]['id']
    context._engine._valid[0] = True
    context.setParameter('a', 3.0)              # an outer global
    assert rec.calls[-1] == ('cv_set_globals', cid, [3.0]) and context._engine._valid[0] is False
    context.setParameter('b', 0.75)             # a derivative parameter
    assert rec.calls[-1] == ('cv_set_variables', cid, [0.75])
    context.setParameter('scale', 0.5)          # an inner global
    assert rec.calls[-1] == ('term_expr_set_globals', tid, [0.5])
    # deriv(energy, b): the kernel's seeded pass; a parameter that was not named is refused by name
    assert context._engine.energy_derivative('b') == 1.0 and rec.calls[-1] == ('cv_energy_derivative', cid, 1)
    with pytest.raises(NotImplementedError, match='did not name the parameter with addEnergyParameterDerivative'):
        context._engine.energy_derivative('a')
    state = context.getState(getParameterDerivatives=True)
    assert state.getEnergyParameterDerivatives()['b'] == 1.0
    # updateParametersInContext: the inner angle text reads its per-term parameters again
    cv.getCollectiveVariable(1).setAngleParameters(0, 0, 1, 2, [310.0, -0.25])
    cv.updateParametersInContext(context)
    last = rec.calls[-1]
    assert last[0] == 'term_expr_set_params' and last[1] == tid and last[2].tolist() == [[310.0], [-0.25]]
    # ... and a force whose inner forces have nothing to reload keeps the refusal
    system = bare_system()
    plain = openmm.CustomCVForce('2*cv1')
    bonds = openmm.HarmonicBondForce()
    bonds.addBond(0, 1, 0.1, 1000.0)
    plain.addCollectiveVariable('cv1', bonds)
    system.addForce(plain)
    context = context_of(system)
    with pytest.raises(NotImplementedError, match='updateParametersInContext for CustomCVForce'):
        plain.updateParametersInContext(context)


def test_the_pattern_of_alchemical_respa_keeps_its_path(recorder, phenol):
    system = system_from_arrays(phenol, nonbondedMethod='PME', cutoff=1.0, switch=0.9)
    solute = [int(i) for i in np.where(phenol['resname'] == 'aaa')[0]]
    alch = atomsmm.AlchemicalRespaSystem(system, 7 * unit.angstroms, 5 * unit.angstroms, solute, coupling_function='lambda^4*(5-4*lambda)')
    context = context_of(alch)
    rec = recorder[-1]
    assert not rec.cvs
    entries = [e for e in context._engine.entries if isinstance(e.force, openmm.CustomCVForce)]
    assert entries and all(e.cv is None and e.pair_ids and not e.term_ids for e in entries)
    with pytest.raises(NotImplementedError, match='its collective variable is never formed'):
        entries[0].force.getCollectiveVariableValues(context)


def test_refusals_by_name(recorder, monkeypatch):
    def system_with(force):
        system = bare_system()
        system.addForce(force)
        return system
    # a pair force outside the old pattern (two collective variables), and a class that is no bonded force
    pair = openmm.CustomNonbondedForce('r')
    for _ in range(8):
        pair.addParticle([])
    cv = openmm.CustomCVForce('u + phi')
    cv.addCollectiveVariable('u', pair)
    cv.addCollectiveVariable('phi', torsion_cv())
    with pytest.raises(NotImplementedError, match='CustomCVForce over a CustomNonbondedForce'):
        context_of(system_with(cv))
    cv = openmm.CustomCVForce('u')
    cv.addCollectiveVariable('u', restraint_force())
    with pytest.raises(NotImplementedError, match='CustomCVForce over a CustomCVForce'):
        context_of(system_with(cv))
    # tabulated functions
    cv = restraint_force()
    cv.addTabulatedFunction('bias', openmm.Continuous1DFunction([0.0, 1.0, 2.0, 3.0], -4.0, 4.0))
    with pytest.raises(NotImplementedError, match='CustomCVForce: tabulated functions'):
        context_of(system_with(cv))
    # a derivative parameter that an inner force's text also reads
    cv = openmm.CustomCVForce('0.5*K*(phi-s)^2')
    inner = torsion_cv('s*theta')
    inner.addGlobalParameter('s', 1.0)
    cv.addCollectiveVariable('phi', inner)
    cv.addGlobalParameter('K', 10.0)
    cv.addGlobalParameter('s', 1.0)
    cv.addEnergyParameterDerivative('s')
    with pytest.raises(NotImplementedError, match='derivative parameter s is also read by the energy expression of collective variable phi'):
        context_of(system_with(cv))
    # a parameter derivative on the inner force itself: the term-expression refusal of old
    cv = openmm.CustomCVForce('phi')
    inner = torsion_cv('g*theta')
    inner.addGlobalParameter('g', 1.0)
    inner.addEnergyParameterDerivative('g')
    cv.addCollectiveVariable('phi', inner)
    with pytest.raises(NotImplementedError, match='no addEnergyParameterDerivative'):
        context_of(system_with(cv))
    # the limits, through the Context
    cv = openmm.CustomCVForce('+'.join('c%d' % k for k in range(17)))
    for k in range(17):
        cv.addCollectiveVariable('c%d' % k, torsion_cv())
    with pytest.raises(atomsmm.InputError, match=r'17 collective variables \(limit 16\)'):
        context_of(system_with(cv))
    # several ranks
    monkeypatch.setattr(E.Engine, '_free_space_mode', staticmethod(lambda system, has_box: False))
    system = system_with(restraint_force())
    with pytest.raises(NotImplementedError, match='runs on a single rank'):
        engine = E.Engine.__new__(E.Engine)
        engine.world, engine.parameters = 2, {}
        engine._translate_cv(system.getForce(0), E._Entry(system.getForce(0), 0))
    # ComputingSystem / PressureComputer
    with pytest.raises(NotImplementedError, match='ComputingSystem / PressureComputer: virial of a CustomCVForce'):
        atomsmm.ComputingSystem(system_with(restraint_force()))
    # the reporter's option stays refused (tests/test_reporters_host.py pins the text); the values come from the force itself
    assert callable(openmm.CustomCVForce.getCollectiveVariableValues)
