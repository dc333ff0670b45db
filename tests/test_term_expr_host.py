"""CPU tests of the term-expression forces (CustomBondForce / CustomAngleForce / CustomTorsionForce / CustomExternalForce with any
energy text): the compiler (expr.compile_term), the interpreter's term leaves -- restated in plain Python, tests/term_expr_cases.py --
against the independent 50-digit evaluator of the TEXT (tests/expr_reference.py, derivative by mpmath.diff), the OpenMM-shaped classes,
the translation and its routes (on a recorder over tests/fake_backend.py), and the inputs the GPU tests use."""
import math

import mpmath
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import expr_reference as R
import term_expr_cases as T
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm, unit
from atomsmm_amd.testing import system_from_arrays
from fake_backend import RecordingContext

HOST = R.Budget(4)          # math.* within 4 ulp, x^n by repeated multiplication
NAMES = {v: k for k, v in X.ALL_OPCODES.items()}


def words(prog):
    return [(NAMES[w & 0xff], w >> 8) for w in prog.code]


# ------------------------------------------------------------------------------------ 1. compile_term: the code
def test_leaves_slots_globals_and_definitions_in_any_order():
    prog = X.compile_term('D*(1-exp(-a*(r-r0)))^2', ('r',), ['D', 'a', 'r0'], [])
    assert words(prog) == [('TERM_P', 0), ('CONST', 0), ('TERM_P', 1), ('NEG', 0), ('TERM_VAR', 0), ('TERM_P', 2), ('SUB', 0), ('MUL', 0),
                           ('exp', 0), ('SUB', 0), ('POWI', 2), ('MUL', 0)] and prog.consts == [1.0] and prog.globals_ == []
    # the three variables of an external force, a global, and a per-term name that shadows nothing
    prog = X.compile_term('k*(x-x0)^2 + g*y*z', ('x', 'y', 'z'), ['k', 'x0'], ['g'])
    assert words(prog) == [('TERM_P', 0), ('TERM_VAR', 0), ('TERM_P', 1), ('SUB', 0), ('POWI', 2), ('MUL', 0), ('GLOBAL', 0), ('TERM_VAR', 1),
                           ('MUL', 0), ('TERM_VAR', 2), ('MUL', 0), ('ADD', 0)] and prog.globals_ == ['g']
    forward = X.compile_term('a*b; a = lambda*theta; b = a + k', ('theta',), ['k'], ['lambda'])
    backward = X.compile_term('a*b; b = a + k; a = lambda*theta', ('theta',), ['k'], ['lambda'])
    assert forward.globals_ == backward.globals_ == ['lambda']
    for prog in (forward, backward):
        e, d = T.run_term_program(prog, [0.5], [3.0], {'lambda': 0.25})
        assert e == 0.125 * 3.125 and d == pytest.approx(0.25 * 3.125 + 0.125 * 0.25, rel=1e-15)
    # a literal definition is folded: the CHARMM improper's pi never becomes a local
    prog = X.compile_term(T.TEXTS['charmm-improper']['text'], ('theta',), ['k', 'theta0'], [])
    assert 2.0 * 3.141592653589793 in prog.consts and sum(1 for w in words(prog) if w[0] == 'STORE') == 1
    # the new words are clear of the pair words and of the shared ones
    assert X.TERM_OPCODES == dict(TERM_VAR=53, TERM_P=54)
    assert not set(X.TERM_OPCODES.values()) & (set(X.OPCODES.values()) | set(X.PAIR_OPCODES.values()))
    # r is no symbol of an angle, theta none of a bond
    with pytest.raises(X.ExpressionError, match='unknown symbol in term expression: r'):
        X.compile_term('k*r', ('theta',), ['k'], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in term expression: theta'):
        X.compile_term('k*theta', ('r',), ['k'], [])
    with pytest.raises(X.ExpressionError, match='random numbers'):
        X.compile_term('r*gaussian', ('r',), [], [])


def test_limits_are_named():
    v = ('r',)
    with pytest.raises(X.ExpressionError, match=r'term expression: stack depth 17 \(limit 16\)'):
        X.compile_term('r' + '+(r' * 16 + ')' * 16, v, [], [])
    X.compile_term('r' + '+(r' * 15 + ')' * 15, v, [], [])
    with pytest.raises(X.ExpressionError, match=r'term expression: \d+ code words \(limit 256\)'):
        X.compile_term('+'.join(['r*r'] * 90), v, [], [])
    with pytest.raises(X.ExpressionError, match=r'term expression: 49 constants \(limit 48\)'):
        X.compile_term('+'.join('%d.5*r' % k for k in range(49)), v, [], [])
    names = ['g%d' % k for k in range(49)]
    with pytest.raises(X.ExpressionError, match=r'term expression: 49 global parameters \(limit 48\)'):
        X.compile_term('r*(' + '+'.join(names) + ')', v, [], names)
    with pytest.raises(X.ExpressionError, match='term expression: more than 16 auxiliary definitions'):
        X.compile_term('+'.join('d%d' % k for k in range(17)) + ';' + ';'.join('d%d = r*%d' % (k, k + 2) for k in range(17)), v, [], [])
    eight = ['p%d' % k for k in range(8)]
    assert [w for w in words(X.compile_term('r*' + '*'.join(eight), v, eight, [])) if w[0] == 'TERM_P'] == [('TERM_P', k) for k in range(8)]
    with pytest.raises(atomsmm.InputError, match=r'at most 8 per-term parameters \(9 given\)'):
        X.compile_term('r*p0', v, eight + ['p8'], [])
    with pytest.raises(X.ExpressionError, match=r'periodicdistance\(\.\.\.\) is not supported'):
        X.compile_term('k*periodicdistance(x, y, z, x0, y0, z0)^2', ('x', 'y', 'z'), ['k', 'x0', 'y0', 'z0'], [])


# ------------------------------------------------------------------------------------ 2. the interpreter's leaves against the evaluator
RANGES = {
    'harmonic-bond': dict(r=(0.08, 0.25), r0=(0.09, 0.2), k=(1e5, 5e5)),
    'harmonic-angle': dict(theta=(0.5, 3.0), theta0=(1.5, 2.2), k=(200.0, 800.0)),
    'periodic-torsion': dict(theta=(-3.1, 3.1), n=(1.0, 4.0), theta0=(0.0, 3.14), k=(0.5, 20.0)),
    'morse': dict(r=(0.08, 0.3), D=(100.0, 500.0), a=(10.0, 25.0), r0=(0.09, 0.2)),
    'morse-global': dict(r=(0.08, 0.3), D=(100.0, 500.0), r0=(0.09, 0.2)),
    'fene': dict(r=(0.05, 0.14), k=(1e3, 3e4), R0=(0.15, 0.3)),
    'cosine-angle': dict(theta=(0.5, 3.0), theta0=(1.5, 2.2), k=(200.0, 800.0)),
    'rb-torsion': dict(theta=(-3.1, 3.1), c0=(-10.0, 10.0), c1=(-10.0, 10.0), c2=(-10.0, 10.0), c3=(-10.0, 10.0), c4=(-10.0, 10.0),
                       c5=(-10.0, 10.0)),
    'charmm-improper': dict(theta=(-3.1, 3.1), k=(10.0, 200.0), theta0=(-3.0, 3.0)),
    'position-restraint': dict(x=(-1.0, 3.0), y=(-1.0, 3.0), z=(-1.0, 3.0), k=(100.0, 1000.0), x0=(0.0, 2.0), y0=(0.0, 2.0), z0=(0.0, 2.0)),
    'flat-bottom': dict(x=(-1.0, 3.0), y=(-1.0, 3.0), z=(-1.0, 3.0), k=(100.0, 1000.0), d0=(0.1, 1.5), x0=(0.0, 2.0), y0=(0.0, 2.0),
                        z0=(0.0, 2.0)),
    'wall': dict(x=(-1.0, 3.0), y=(-1.0, 3.0), z=(0.0, 3.0), m=(1.0, 40.0)),
}


@pytest.mark.parametrize('name', sorted(T.TEXTS))
def test_program_matches_the_independent_evaluator(name):
    """A dozen texts over every variable set: E within the bound of a double evaluation, every partial derivative to 1e-9."""
    case = T.TEXTS[name]
    variables = T.VARIABLES[case['kind']]
    prog = X.compile_term(case['text'], variables, case['names'], case['globals'])
    main, defs = R.parse(case['text'])
    rng = np.random.default_rng(sum(map(ord, name)))
    done = replaced = 0
    worst_d = 0.0
    while done < 60:
        draw = {s: float(rng.uniform(*RANGES[name][s])) for s in list(variables) + case['names']}
        if name == 'periodic-torsion':
            draw['n'] = float(round(draw['n']))
        g = {k: float(v * rng.uniform(0.8, 1.2)) for k, v in case['globals'].items()}
        v, p = [draw[s] for s in variables], [draw[s] for s in case['names']]
        if not all(abs(q) > T.KINK_MARGIN for q in case['kinks'](v, p, g)):
            replaced += 1
            continue
        env = dict(g, **draw)
        try:
            with mpmath.workdps(R.DIGITS):
                value, bound = R._evaluate_one(main, defs, env, HOST)
                slopes = [mpmath.diff(lambda c, s=s: R._evaluate_one(main, defs, dict(env, **{s: c}), R.NO_ROUNDING)[0], mpmath.mpf(env[s]))
                          for s in variables]
        except R.Unstable:
            replaced += 1
            continue
        for k, slope in enumerate(slopes):
            e, d = T.run_term_program(prog, v, p, g, seed=k)
            assert abs(e - value) <= bound, (draw, g, e, float(value))
            scale = max(abs(s) for s in slopes)
            if scale == 0:
                assert d == 0.0
            else:
                assert abs(d - slope) <= 1e-9 * scale, (draw, g, k, d, float(slope))
                worst_d = max(worst_d, float(abs(d - slope) / scale))
        done += 1
    print('%s: %d code words, worst derivative error %.2e of the largest partial, %d draws replaced' % (name, len(prog.code), worst_d, replaced))
    assert replaced <= 0.2 * (done + replaced)


def test_flat_bottom_at_its_anchor_has_zero_derivative():
    """d = sqrt(0): f' = inf, but the sum of squares has derivative exactly zero there -- an exact zero, not NaN."""
    case = T.TEXTS['flat-bottom']
    prog = X.compile_term(case['text'], ('x', 'y', 'z'), case['names'], {})
    for k in range(3):
        assert T.run_term_program(prog, [0.5, 0.25, 1.0], [300.0, 0.2, 0.5, 0.25, 1.0], {}, seed=k) == (0.0, 0.0)


# ------------------------------------------------------------------------------------ 3. the OpenMM-shaped classes
def test_new_classes_and_setters():
    t = openmm.CustomTorsionForce('k*theta^2')
    assert t.addPerTorsionParameter('k') == 0 and t.getNumPerTorsionParameters() == 1 and t.getPerTorsionParameterName(0) == 'k'
    assert t.addTorsion(0, 1, 2, 3, [2.0 * unit.kilojoules_per_mole]) == 0 and t.getNumTorsions() == 1
    assert t.getTorsionParameters(0) == [0, 1, 2, 3, (2.0,)]
    t.setTorsionParameters(0, 3, 2, 1, 0, [5.0])
    assert t.getTorsionParameters(0) == [3, 2, 1, 0, (5.0,)]
    assert t.addGlobalParameter('g', 1.5) == 0 and t.getGlobalParameterDefaultValue(0) == 1.5
    assert t.usesPeriodicBoundaryConditions() is False
    t.setUsesPeriodicBoundaryConditions(True)
    assert t.usesPeriodicBoundaryConditions() is True and t.getEnergyFunction() == 'k*theta^2'
    x = openmm.CustomExternalForce('k*z')
    assert x.addPerParticleParameter('k') == 0 and x.getNumPerParticleParameters() == 1 and x.getPerParticleParameterName(0) == 'k'
    assert x.addParticle(7, [3.0]) == 0 and x.getNumParticles() == 1 and x.getParticleParameters(0) == [7, (3.0,)]
    x.setParticleParameters(0, 5, [4.0])
    assert x.getParticleParameters(0) == [5, (4.0,)] and x.usesPeriodicBoundaryConditions() is False
    a = openmm.CustomAngleForce('k*theta')
    a.addPerAngleParameter('k')
    a.addAngle(0, 1, 2, [1.0])
    a.setAngleParameters(0, 2, 1, 0, [2.0])
    a.setEnergyFunction('2*k*theta')
    assert a.getAngleParameters(0) == [2, 1, 0, (2.0,)] and a.getEnergyFunction() == '2*k*theta'
    for cls in (openmm.CustomBondForce, openmm.CustomAngleForce, openmm.CustomTorsionForce, openmm.CustomExternalForce):
        assert callable(getattr(cls, 'updateParametersInContext'))
    # the alias packages see them like their neighbours
    import atomsmm.systems
    from simtk import openmm as simtk_openmm
    for view in (simtk_openmm, atomsmm.systems.openmm):
        assert view.CustomTorsionForce is openmm.CustomTorsionForce and view.CustomExternalForce is openmm.CustomExternalForce


def test_molecules_follow_custom_torsions_and_ignore_external_forces():
    system = openmm.System()
    for _ in range(7):
        system.addParticle(1.0)
    t = openmm.CustomTorsionForce('theta')
    t.addTorsion(0, 1, 2, 3)
    x = openmm.CustomExternalForce('x')
    x.addParticle(4)
    x.addParticle(5)
    system.addForce(t)
    system.addForce(x)
    assert openmm.molecules_of(system) == [[0, 1, 2, 3], [4], [5], [6]]


# ------------------------------------------------------------------------------------ 4. the translation and its routes
class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.terms, self.added = [], []

    def bonded_add_terms(self, fid, kind, idx, params, periodic=False, desc=None):
        RecordingContext.bonded_add_terms(self, fid, kind, idx, params, periodic, desc)
        self.added.append(dict(id=fid, kind=kind, idx=np.array(idx), params=np.array(params), periodic=bool(periodic), desc=desc))

    def term_expr_create(self, kind, code, consts, globals_, idx, params, periodic=False):
        fid = self._new()
        self.terms.append(dict(id=fid, kind=kind, code=list(code), consts=list(consts), globals=list(globals_), idx=np.array(idx),
                               params=np.array(params), periodic=bool(periodic)))
        return fid

    def term_expr_set_globals(self, fid, globals_):
        self.calls.append(('term_expr_set_globals', fid, list(globals_)))

    def term_expr_set_params(self, fid, params, n_terms):
        self.calls.append(('term_expr_set_params', fid, np.array(params), n_terms))


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


def morse_force(periodic=False):
    force = openmm.CustomBondForce('D*(1-exp(-a*(r-r0)))^2')
    for name in ('D', 'a', 'r0'):
        force.addPerBondParameter(name)
    for k in range(3):
        force.addBond(k, k + 1, [100.0 + k, 20.0 + k, 0.1 + 0.01 * k])
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


def test_recognised_texts_keep_their_routes(recorder, emim):
    # redefine_bond / redefine_angle: two harmonic sets each, +K0 at the old value and -Kn at the new one
    system = bare_system()
    bond = openmm.CustomBondForce('0.5*(K0*(r - r0)^2 - Kn*(r - rn)^2)')
    for name in ('r0', 'K0', 'rn', 'Kn'):
        bond.addPerBondParameter(name)
    bond.addBond(0, 1, [0.1, 1000.0, 0.11, 900.0])
    angle = openmm.CustomAngleForce('0.5*(K0*(theta - t0)^2 - Kn*(theta - tn)^2)')
    for name in ('t0', 'K0', 'tn', 'Kn'):
        angle.addPerAngleParameter(name)
    angle.addAngle(0, 1, 2, [1.9, 300.0, 1.8, 250.0])
    virial = openmm.CustomBondForce('-K*r*(r-r0)')
    for name in ('r0', 'K'):
        virial.addPerBondParameter(name)
    virial.addBond(2, 3, [0.1, 1000.0])
    for k, force in enumerate((bond, angle, virial)):
        force.setForceGroup(k)
        system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    assert not rec.terms and not any(e.term_expr or e.term_ids for e in context._engine.entries)
    got = [(a['kind'], a['idx'].tolist(), a['params'].tolist(), a['periodic']) for a in rec.added]
    assert got == [(B.BOND_HARMONIC, [[0, 1]], [[0.1, 1000.0]], False), (B.BOND_HARMONIC, [[0, 1]], [[0.11, -900.0]], False),
                   (B.ANGLE_HARMONIC, [[0, 1, 2]], [[1.9, 300.0]], False), (B.ANGLE_HARMONIC, [[0, 1, 2]], [[1.8, -250.0]], False),
                   (B.BOND_VIRIAL_HARMONIC, [[2, 3]], [[0.1, 1000.0]], False)]
    # the exception forces of RESPASystem: ljc (fastExceptions) and near
    for fast, kind in ((True, B.BOND_LJC), (False, B.BOND_NEAR)):
        respa = atomsmm.RESPASystem(system_from_arrays(emim), 0.7 * unit.nanometers, 0.5 * unit.nanometers, fastExceptions=fast)
        context = context_of(respa)
        rec = recorder[-1]
        assert not rec.terms
        custom = [e for e in context._engine.entries if isinstance(e.force, openmm.CustomBondForce)]
        assert custom and all(not e.term_expr and [t[0] for t in e.terms] == [kind] for e in custom)
        mine = [a for a in rec.added if a['kind'] == kind]
        assert len(mine) == len(custom) == (1 if fast else 2)
        for a in mine:          # every exception with its raw (chargeprod, sigma, epsilon), periodic, with the family's descriptor
            assert np.array_equal(a['idx'], emim['exc_pairs']) and a['periodic'] is True and a['desc'] is not None
            assert np.array_equal(a['params'], np.stack([emim['exc_chargeprod'], emim['exc_sigma'], emim['exc_epsilon']], axis=1))


def test_generic_texts_take_the_term_expression_route(recorder):
    system = bare_system()
    morse = morse_force(periodic=True)
    angle = openmm.CustomAngleForce('0.5*k*(theta-theta0)^2')
    angle.addPerAngleParameter('theta0')
    angle.addPerAngleParameter('k')
    angle.addAngle(0, 1, 2, [1.9, 300.0])
    angle.addAngle(1, 2, 3, [1.8, 310.0])
    rb = openmm.CustomTorsionForce(T.TEXTS['rb-torsion']['text'])
    for name in T.TEXTS['rb-torsion']['names']:
        rb.addPerTorsionParameter(name)
    rb.addTorsion(0, 1, 2, 3, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    rb.addTorsion(4, 5, 6, 7, [7.0, 8.0, 9.0, 10.0, 11.0, 12.0])
    restraint = openmm.CustomExternalForce('0.5*kr*scale*((x-x0)^2+(y-y0)^2+(z-z0)^2)')
    restraint.addGlobalParameter('scale', 1.0)
    restraint.addGlobalParameter('unused', 3.0)
    for name in ('kr', 'x0', 'y0', 'z0'):
        restraint.addPerParticleParameter(name)
    restraint.addParticle(5, [1000.0, 0.1, 0.2, 0.3])
    restraint.addParticle(2, [900.0, 0.4, 0.5, 0.6])
    for force in (morse, angle, rb, restraint):
        system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    assert not rec.added and [t['kind'] for t in rec.terms] == [B.TERM_BOND, B.TERM_ANGLE, B.TERM_TORSION, B.TERM_EXTERNAL] == [0, 1, 2, 3]
    m, a, t, x = rec.terms
    # index rows padded with -1, values parameter-major
    assert m['idx'].tolist() == [[0, 1, -1, -1], [1, 2, -1, -1], [2, 3, -1, -1]] and m['periodic'] is True
    assert m['params'].tolist() == [[100.0, 101.0, 102.0], [20.0, 21.0, 22.0], [0.1, 0.1 + 0.01 * 1, 0.1 + 0.01 * 2]]
    assert a['idx'].tolist() == [[0, 1, 2, -1], [1, 2, 3, -1]] and a['params'].tolist() == [[1.9, 1.8], [300.0, 310.0]] and not a['periodic']
    assert t['idx'].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]] and t['params'].shape == (6, 2) and t['params'][:, 1].tolist() == [7.0, 8.0, 9.0, 10.0, 11.0, 12.0]
    assert x['idx'].tolist() == [[5, -1, -1, -1], [2, -1, -1, -1]] and x['params'].tolist() == [[1000.0, 900.0], [0.1, 0.4], [0.2, 0.5], [0.3, 0.6]]
    assert x['periodic'] is False and x['globals'] == [1.0]          # the globals the program reads, in its order
    entries = context._engine.entries
    assert all(e.term_expr and e.term_ids == [rec.terms[k]['id']] and e.bonded_id is None and not e.terms for k, e in enumerate(entries))
    assert list(entries[0].program.code) == m['code'] and entries[3].depends == {'scale'} and entries[0].update is None
    # setParameter -> set_globals; a parameter the program does not read changes nothing
    context.setParameter('scale', 0.5)
    assert rec.calls[-1] == ('term_expr_set_globals', x['id'], [0.5])
    before = len(rec.calls)
    context.setParameter('unused', 4.0)
    assert not [c for c in rec.calls[before:] if c[0].startswith('term_expr')]
    # updateParametersInContext -> set_params with all values again
    morse.setBondParameters(1, 1, 2, [150.0, 25.0, 0.2])
    morse.updateParametersInContext(context)
    call = rec.calls[-1]
    assert call[0] == 'term_expr_set_params' and call[1] == m['id'] and call[3] == 3
    assert call[2].tolist() == [[100.0, 150.0, 102.0], [20.0, 25.0, 22.0], [0.1, 0.2, 0.1 + 0.01 * 2]]
    restraint.setParticleParameters(1, 2, [800.0, 0.4, 0.5, 0.6])
    restraint.updateParametersInContext(context)
    assert rec.calls[-1][0] == 'term_expr_set_params' and rec.calls[-1][2][0].tolist() == [1000.0, 800.0]
    # changed atoms or numbers: OpenMM's error
    morse.setBondParameters(1, 1, 3, [150.0, 25.0, 0.2])
    with pytest.raises(openmm.OpenMMException, match='the particles of the bonds have changed'):
        morse.updateParametersInContext(context)
    rb.addTorsion(0, 1, 2, 3, [0.0] * 6)
    with pytest.raises(openmm.OpenMMException, match='the number of torsions has changed'):
        rb.updateParametersInContext(context)
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, scale\) of a CustomExternalForce with a generic energy expression'):
        context._engine.energy_derivative('scale')


def test_group_ids_end_with_the_term_expression_ids(recorder, emim):
    system = system_from_arrays(emim)          # HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce, NonbondedForce: group 0
    rb = openmm.CustomTorsionForce('k*theta^2')
    rb.addPerTorsionParameter('k')
    rb.addTorsion(0, 1, 2, 3, [1.0])
    system._forces.insert(0, rb)               # (translated first: the lowest backend id, and still the last but one of the group)
    pin = openmm.CustomExternalForce('x^2')
    pin.addParticle(0)
    system.addForce(pin)
    context = context_of(system)
    rec = recorder[-1]
    engine = context._engine
    engine._define_group(0)
    slot, ids = rec.groups[0]
    term_ids = [t['id'] for t in rec.terms]
    assert len(term_ids) == 2 and ids[-2:] == term_ids and len(ids) >= 4
    # pair forces first, then the merged bond-list set (the recorder numbers objects as they are made)
    pair_ids = [pid for e in engine.entries for pid in e.pair_ids]
    assert ids[:len(pair_ids)] == pair_ids and ids[len(pair_ids)] == rec.bonded[-1]['id']


def test_clean_refusals(recorder):
    def job(rank):
        system = bare_system()
        system.addForce(morse_force())
        with pytest.raises(NotImplementedError, match='CustomBondForce: energy expression not recognised.*runs on a single rank'):
            context_of(system)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
    # addEnergyParameterDerivative through any of the four classes
    for cls, variable in ((openmm.CustomBondForce, 'r'), (openmm.CustomAngleForce, 'theta'), (openmm.CustomTorsionForce, 'theta'),
                          (openmm.CustomExternalForce, 'x')):
        system = bare_system()
        force = cls('k*' + variable)
        force.addGlobalParameter('k', 1.0)
        force.addEnergyParameterDerivative('k')
        system.addForce(force)
        with pytest.raises(NotImplementedError, match=cls.__name__ + '.*addEnergyParameterDerivative'):
            context_of(system)
    system = bare_system()
    force = openmm.CustomAngleForce('k*theta*zeta')
    force.addPerAngleParameter('k')
    system.addForce(force)
    with pytest.raises(atomsmm.InputError, match='CustomAngleForce.*unknown symbol in term expression: zeta'):
        context_of(system)
    system = bare_system()
    force = openmm.CustomExternalForce('k*periodicdistance(x, y, z, 0, 0, 0)^2')
    force.addPerParticleParameter('k')
    system.addForce(force)
    with pytest.raises(atomsmm.InputError, match=r'periodicdistance\(\.\.\.\) is not supported'):
        context_of(system)
    system = bare_system()
    force = openmm.CustomBondForce('r*' + '*'.join('p%d' % k for k in range(9)))
    for k in range(9):
        force.addPerBondParameter('p%d' % k)
    system.addForce(force)
    with pytest.raises(atomsmm.InputError, match=r'at most 8 per-term parameters \(9 given\)'):
        context_of(system)
    system = bare_system()
    force = morse_force()
    force.addBond(0, 99, [1.0, 1.0, 1.0])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='particle index is out of range'):
        context_of(system)
    system = bare_system()
    force = morse_force()
    force.addBond(0, 5, [1.0, 1.0])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='needs 3 parameters'):
        context_of(system)
    # free space: allowed without the flag, refused with it
    system = bare_system(box=False)
    system.addForce(morse_force())
    context_of(system)
    assert recorder[-1].terms[0]['periodic'] is False and recorder[-1].box is None
    system = bare_system(box=False)
    nb = openmm.NonbondedForce()
    for _ in range(8):
        nb.addParticle(0.0, 0.3, 0.5)
    nb.setNonbondedMethod(nb.NoCutoff)
    system.addForce(nb)
    system.addForce(morse_force(periodic=True))
    with pytest.raises(atomsmm.InputError, match='periodic boundary'):
        context_of(system)


# ------------------------------------------------------------------------------------ 5. the inputs of the GPU references
def test_gpu_reference_inputs_are_usable(emim):
    """The terms test_gpu_term_expr.py compares against term_expr_cases.term_sum: none is an input to avoid, none raises Unstable."""
    for name in T.GPU_CASES:
        case = T.TEXTS[name]
        idx, params = T.reference_terms(name, emim)
        assert len(idx) >= 24
        box = emim['box']
        for atoms, p in zip(idx, params):
            assert T.usable(case, emim['positions'], atoms, p, box)
        # (the first flat-bottom term sits exactly at its anchor, as the GPU test wants it: sqrt(0) is on the edge of its domain, the
        # energy is identically zero around it -- the reference there is the exact zero, checked by the GPU test itself)
        first = 1 if name == 'flat-bottom' else 0
        assert name != 'flat-bottom' or np.array_equal(params[0][2:5], emim['positions'][idx[0][0]])
        for atoms, p in list(zip(idx, params))[first:]:
            T.exact_term(case, emim['positions'], atoms, p, box, budget=HOST, forces=False)
