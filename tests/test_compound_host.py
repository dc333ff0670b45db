"""CPU tests of the compound-bond forces (CustomCompoundBondForce / CustomCentroidBondForce with any energy text): the compiler
(expr.compile_compound) and its variable table, the compiled programs -- run through the plain-Python restatement of the interpreter,
tests/term_expr_cases.py -- against the independent 50-digit evaluator of the TEXT (tests/compound_cases.py), the OpenMM-shaped
classes, the translation and its routes (on a recorder over tests/fake_backend.py), and the words of every text the earlier host tests
compile against the parent's (tests/golden/expr_words_parent.json)."""
import json
import os

import mpmath
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import compound_cases as C
import expr_reference as R
import term_expr_cases as T
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm
from fake_backend import RecordingContext

HOST = R.Budget(4)          # math.* within 4 ulp, x^n by repeated multiplication
NAMES = {v: k for k, v in X.ALL_OPCODES.items()}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def words(prog):
    return [(NAMES[w & 0xff], w >> 8) for w in prog.code]


# ------------------------------------------------------------------------------------ 1. compile_compound: the code and the table
def test_variable_table_and_words_of_three_texts():
    prog, table = X.compile_compound('0.5*k*(angle(p1,p2,p3)-t0)^2 + 0.5*kub*(distance(p1,p3)-d0)^2', 3, 'p', ['t0', 'k', 'd0', 'kub'], [])
    assert table == [('angle', (0, 1, 2)), ('distance', (0, 2))]
    assert words(prog) == [('CONST', 0), ('TERM_P', 1), ('MUL', 0), ('TERM_VAR', 0), ('TERM_P', 0), ('SUB', 0), ('POWI', 2), ('MUL', 0),
                           ('CONST', 0), ('TERM_P', 3), ('MUL', 0), ('TERM_VAR', 1), ('TERM_P', 2), ('SUB', 0), ('POWI', 2), ('MUL', 0), ('ADD', 0)]
    assert prog.consts == [0.5] and prog.globals_ == []
    # raw coordinates, a global, a definition; the centroid class says g, and x1 is the centre of group 1
    prog, table = X.compile_compound('s*(d - z2 + x1); d = distance(g2,g1)', 2, 'g', [], ['s', 'unused'])
    assert table == [('distance', (1, 0)), ('z', (1,)), ('x', (0,))] and prog.globals_ == ['s']
    assert words(prog) == [('GLOBAL', 0), ('TERM_VAR', 0), ('STORE', 0), ('LOAD', 0), ('TERM_VAR', 1), ('SUB', 0), ('TERM_VAR', 2), ('ADD', 0),
                           ('MUL', 0)]
    prog, table = X.compile_compound('k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0))', 4, 'p', ['n', 't0', 'k'], [])
    assert table == [('dihedral', (0, 1, 2, 3))]
    assert words(prog) == [('TERM_P', 2), ('CONST', 0), ('TERM_P', 0), ('TERM_VAR', 0), ('MUL', 0), ('TERM_P', 1), ('SUB', 0), ('cos', 0),
                           ('ADD', 0), ('MUL', 0)]
    # ... the words of the same text as a CustomTorsionForce
    assert prog.code == X.compile_term('k*(1+cos(n*theta-t0))', ('theta',), ['n', 't0', 'k'], []).code


def test_identical_calls_share_a_variable():
    prog, table = X.compile_compound('distance(p1,p2)*distance(p1,p2) + distance(p2,p1) + x1*x1 + angle(p1,p2,p3) - angle(p1, p2, p3)', 3, 'p', [], [])
    assert table == [('distance', (0, 1)), ('distance', (1, 0)), ('x', (0,)), ('angle', (0, 1, 2))]
    assert [w for w in words(prog) if w[0] == 'TERM_VAR'] == [('TERM_VAR', k) for k in (0, 0, 1, 2, 2, 3, 3)]
    # the sixteen-variable text of the GPU tests: all four kinds, the raw coordinates of the eighth particle among them
    prog, table = X.compile_compound(C.TEXTS['sixteen']['text'], 8, 'p', C.TEXTS['sixteen']['names'], C.TEXTS['sixteen']['globals'])
    assert len(table) == 16 and {k for k, _ in table} == {'x', 'y', 'z', 'distance', 'angle', 'dihedral'}
    assert ('x', (7,)) in table and ('y', (7,)) in table and ('z', (7,)) in table
    for name, count in C.N_VARIABLES.items():
        case = C.TEXTS[name]
        prefix = 'g' if name.startswith('centre') else 'p'
        assert len(X.compile_compound(case['text'], case['n'], prefix, case['names'], case['globals'])[1]) == count


def test_limits_and_refused_names_are_named():
    with pytest.raises(atomsmm.InputError, match=r'1 to 8 particles per bond \(9 given\)'):
        X.compile_compound('x9', 9, 'p', [], [])
    with pytest.raises(atomsmm.InputError, match=r'1 to 8 groups per bond \(9 given\)'):
        X.compile_compound('x9', 9, 'g', [], [])
    X.compile_compound('x8', 8, 'p', [], [])
    eight = ['q%d' % k for k in range(8)]
    X.compile_compound('x1*' + '*'.join(eight), 1, 'p', eight, [])
    with pytest.raises(atomsmm.InputError, match=r'at most 8 per-bond parameters \(9 given\)'):
        X.compile_compound('x1', 1, 'p', eight + ['q8'], [])
    sixteen = '+'.join('%s%d' % (a, k) for k in range(1, 7) for a in 'xyz')[:-len('+y6+z6')]
    assert len(X.compile_compound(sixteen, 6, 'p', [], [])[1]) == 16
    with pytest.raises(X.ExpressionError, match='more than 16 distinct geometric variables'):
        X.compile_compound(sixteen + '+distance(p1,p2)', 6, 'p', [], [])
    for fn in ('pointdistance', 'pointangle', 'pointdihedral'):
        with pytest.raises(X.ExpressionError, match=fn + r'\(\.\.\.\) is not supported in a compound-bond expression'):
            X.compile_compound('%s(x1,y1,z1,0,0,0)' % fn, 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='arguments of distance are bare names of particles'):
        X.compile_compound('distance(p1, p2+1)', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='arguments of angle are bare names of groups'):
        X.compile_compound('angle(g1, 2, g3)', 3, 'g', [], [])
    with pytest.raises(X.ExpressionError, match='p3 is none of the particles of a bond'):
        X.compile_compound('distance(p1, p3)', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='g1 is none of the particles of a bond'):
        X.compile_compound('distance(p1, g1)', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match=r'dihedral takes 4 particles \(3 given\)'):
        X.compile_compound('dihedral(p1, p2, p3)', 4, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='p1 names one of the particles; it stands only as an argument'):
        X.compile_compound('2*p1', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in compound-bond expression: x3'):
        X.compile_compound('x3', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='the parameter x1 shadows the coordinate'):
        X.compile_compound('x1', 2, 'p', ['x1'], [])
    # the program limits of a pair expression hold, under this kind's name
    with pytest.raises(X.ExpressionError, match=r'compound-bond expression: stack depth 17 \(limit 16\)'):
        X.compile_compound('x1' + '+(x1' * 16 + ')' * 16, 1, 'p', [], [])
    with pytest.raises(X.ExpressionError, match=r'compound-bond expression: \d+ code words \(limit 256\)'):
        X.compile_compound('+'.join(['x1*x1'] * 90), 1, 'p', [], [])
    with pytest.raises(X.ExpressionError, match=r'periodicdistance\(\.\.\.\) is not supported'):
        X.compile_compound('periodicdistance(x1,y1,z1,x2,y2,z2)', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match='random numbers'):
        X.compile_compound('x1*gaussian', 1, 'p', [], [])


# ------------------------------------------------------------------------------------ 2. the programs against the evaluator
@pytest.mark.parametrize('name', sorted(C.TEXTS))
def test_program_matches_the_independent_evaluator(name, emim):
    """Every text over bonds of the emim fixture: E of the program at the fp64 variables within the bound of a double evaluation of
    the 50-digit energy, every dE/dvariable to 1e-9 of the largest."""
    case = C.TEXTS[name]
    centroid = name.startswith('centre')
    prog, table = X.compile_compound(case['text'], case['n'], 'g' if centroid else 'p', case['names'], case['globals'])
    text, found = C.variables_in(case['text'])
    by_entry = {entry: fresh for fresh, entry in found.items()}
    assert sorted(by_entry) == sorted(table)          # the regular expression and the compiler see the same variables
    order = [by_entry[entry] for entry in table]
    main, defs = R.parse(text)
    pos, box = emim['positions'], emim['box']
    if centroid:
        rng = np.random.default_rng(3)
        rows = [[(list(range(40 * (3 * b + s), 40 * (3 * b + s) + 5)), list(rng.uniform(1.0, 16.0, 5))) for s in range(case['n'])] for b in range(12)]
        params = np.stack([rng.uniform(50.0, 500.0, 12), rng.uniform(0.5, 2.0, 12)], axis=1)
    else:
        rows, params, looked = C.fixture_rows(name, emim, 12)
        assert len(rows) >= C.MIN_KEPT * looked
    worst = 0.0
    for members, p in zip(rows, params):
        assert C.usable(case, pos, members, p, box)
        env = dict(case['globals'], **{q: float(v) for q, v in zip(case['names'], p)})
        values = C.float_variables(case, pos, members, box)
        with mpmath.workdps(R.DIGITS):
            value, bound = R._evaluate_one(main, defs, dict(env, **values), HOST)
            slopes = [mpmath.diff(lambda c, s=s: R._evaluate_one(main, defs, dict(env, **dict(values, **{s: c})), R.NO_ROUNDING)[0],
                                  mpmath.mpf(values[s])) for s in order]
        scale = max(abs(s) for s in slopes)
        for k in range(len(order)):
            e, d = T.run_term_program(prog, [values[s] for s in order], list(p), case['globals'], seed=k)
            assert abs(e - value) <= bound
            assert abs(d - slopes[k]) <= 1e-9 * scale
            worst = max(worst, float(abs(d - slopes[k]) / scale))
        # ... and the fp64 variables themselves are those of the 50-digit reference
        _, _, exact = C.exact_bond(case, pos, members, p, box, forces=False)
        assert all(abs(values[s] - float(exact[s])) <= 1e-12 * max(1.0, abs(values[s])) for s in order)
    print('%s: %d variables, %d code words, worst derivative error %.2e of the largest partial' % (name, len(order), len(prog.code), worst))


def test_reference_forces_are_those_of_a_closed_form():
    """The checker checked: a harmonic bond between two centres in closed form -- F on atom i of group 1 is -k (d - d0) (w_i / W) u."""
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.0, 2.0, (7, 3))
    g1, g2 = ([0, 1, 2], [1.0, 2.0, 0.0]), ([3, 4, 5, 6], [12.0, 1.0, 16.0, 1.0])
    e, f, v = C.exact_bond(C.TEXTS['centre-distance'], pos, [g1, g2], [300.0, 0.4])
    c1, c2 = C.centre(pos, *g1), C.centre(pos, *g2)
    d = np.linalg.norm(c1 - c2)
    assert float(e) == pytest.approx(150.0 * (d - 0.4) ** 2, rel=1e-13) and float(v['distance_1_2']) == pytest.approx(d, rel=1e-14)
    on_c1 = -300.0 * (d - 0.4) * (c1 - c2) / d
    for a, w in zip(*g1):
        assert np.allclose(f[a], w / 3.0 * on_c1, rtol=1e-12, atol=1e-12)
    for a, w in zip(*g2):
        assert np.allclose(f[a], -w / 30.0 * on_c1, rtol=1e-12, atol=1e-12)
    assert not f[2].any()          # weight zero: no force


# ------------------------------------------------------------------------------------ 3. the OpenMM-shaped classes
def test_classes_and_setters():
    f = openmm.CustomCompoundBondForce(3, 'k*angle(p1,p2,p3)')
    assert f.getNumParticlesPerBond() == 3 and f.addPerBondParameter('k') == 0 and f.getNumPerBondParameters() == 1
    assert f.getPerBondParameterName(0) == 'k' and f.addGlobalParameter('g', 2.0) == 0
    assert f.addBond([0, 1, 2], [5.0]) == 0 and f.getNumBonds() == 1 and f.getBondParameters(0) == [(0, 1, 2), (5.0,)]
    f.setBondParameters(0, [2, 1, 0], [6.0])
    assert f.getBondParameters(0) == [(2, 1, 0), (6.0,)] and f.usesPeriodicBoundaryConditions() is False
    f.setUsesPeriodicBoundaryConditions(True)
    assert f.usesPeriodicBoundaryConditions() is True and f.getEnergyFunction() == 'k*angle(p1,p2,p3)'
    with pytest.raises(openmm.OpenMMException, match=r'a bond takes 3 particles \(2 given\)'):
        f.addBond([0, 1], [1.0])
    assert f.addTabulatedFunction('t', openmm.Continuous1DFunction([0.0, 1.0, 2.0], 0.0, 1.0)) == 0 and f.getNumTabulatedFunctions() == 1
    f.addEnergyParameterDerivative('g')
    assert f.getNumEnergyParameterDerivatives() == 1
    c = openmm.CustomCentroidBondForce(2, 'distance(g1,g2)')
    assert c.getNumGroupsPerBond() == 2 and c.addGroup([0, 1, 2]) == 0 and c.addGroup([3, 4], [1.0, 2.0]) == 1 and c.getNumGroups() == 2
    assert c.getGroupParameters(0) == [(0, 1, 2), ()] and c.getGroupParameters(1) == [(3, 4), (1.0, 2.0)]
    c.setGroupParameters(1, [3, 4], [2.0, 2.0])
    assert c.getGroupParameters(1) == [(3, 4), (2.0, 2.0)] and c.addBond([0, 1]) == 0 and c.getBondParameters(0) == [(0, 1), ()]
    with pytest.raises(openmm.OpenMMException, match='one weight per particle'):
        c.addGroup([0, 1], [1.0])
    for cls in (openmm.CustomCompoundBondForce, openmm.CustomCentroidBondForce):
        assert callable(getattr(cls, 'updateParametersInContext'))


def test_molecules_follow_compound_bonds_and_ignore_centroid_bonds():
    system = openmm.System()
    for _ in range(9):
        system.addParticle(1.0)
    f = openmm.CustomCompoundBondForce(3, 'angle(p1,p2,p3)')
    f.addBond([0, 2, 4])
    c = openmm.CustomCentroidBondForce(2, 'distance(g1,g2)')
    c.addGroup([5, 6])
    c.addGroup([7, 8])
    c.addBond([0, 1])
    system.addForce(f)
    system.addForce(c)
    assert openmm.molecules_of(system) == [[0, 2, 4], [1], [3], [5], [6], [7], [8]]


# ------------------------------------------------------------------------------------ 4. the translation and its routes
class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.compounds = []

    def compound_create(self, n_slots, code, consts, globals_, var_kinds, var_slots, idx, params, periodic=False, groups=None):
        fid = self._new()
        self.compounds.append(dict(id=fid, n_slots=n_slots, code=list(code), consts=list(consts), globals=list(globals_), kinds=list(var_kinds),
                                   slots=[list(s) for s in var_slots], idx=np.array(idx), params=np.array(params), periodic=bool(periodic),
                                   groups=None if groups is None else [np.array(g) for g in groups]))
        return fid

    def compound_set_globals(self, fid, globals_):
        self.calls.append(('compound_set_globals', fid, list(globals_)))

    def compound_set_params(self, fid, params, n_bonds):
        self.calls.append(('compound_set_params', fid, np.array(params), n_bonds))

    def compound_set_weights(self, fid, weights):
        self.calls.append(('compound_set_weights', fid, np.array(weights)))

    def cv_create(self, inner_ids, n_deriv, code, consts, globals_):
        fid = self._new()
        self.calls.append(('cv_create', fid, list(inner_ids)))
        return fid


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def bare_system(n=10, box=True):
    system = openmm.System()
    for k in range(n):
        system.addParticle(1.0 + k)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    return system


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


def urey_bradley(periodic=False):
    case = C.TEXTS['urey-bradley']
    force = openmm.CustomCompoundBondForce(3, 'scale*(' + case['text'] + ')')
    for name in case['names']:
        force.addPerBondParameter(name)
    force.addGlobalParameter('scale', 1.0)
    force.addGlobalParameter('unused', 3.0)
    force.addBond([0, 1, 2], [1.9, 300.0, 0.16, 2000.0])
    force.addBond([2, 3, 4], [1.8, 310.0, 0.17, 2100.0])
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


def centroid_restraint(periodic=False):
    force = openmm.CustomCentroidBondForce(2, '0.5*k*(distance(g1,g2)-d0)^2')
    force.addPerBondParameter('k')
    force.addGlobalParameter('d0', 0.5)
    force.addGroup([0, 1, 2])                      # the masses: 1, 2, 3
    force.addGroup([3, 4], [1.0, 0.0])
    force.addGroup([2, 5, 6], [2.0, 2.0, 4.0])
    force.addBond([0, 1], [100.0])
    force.addBond([2, 0], [200.0])
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


def test_both_classes_take_the_compound_route(recorder):
    system = bare_system()
    ub, cr = urey_bradley(periodic=True), centroid_restraint()
    cr.setForceGroup(1)
    system.addForce(ub)
    system.addForce(cr)
    context = context_of(system)
    rec = recorder[-1]
    u, c = rec.compounds
    prog, table = X.compile_compound(ub.getEnergyFunction(), 3, 'p', C.TEXTS['urey-bradley']['names'], ['scale', 'unused'])
    assert u['n_slots'] == 3 and u['code'] == list(prog.code) and u['consts'] == prog.consts and u['globals'] == [1.0] and u['periodic'] is True
    assert u['kinds'] == [B.CVAR_ANGLE, B.CVAR_DISTANCE] == [4, 3] and u['slots'] == [[0, 1, 2], [0, 2]] and u['groups'] is None
    assert u['idx'].tolist() == [[0, 1, 2], [2, 3, 4]] and u['params'].tolist() == [[1.9, 1.8], [300.0, 310.0], [0.16, 0.17], [2000.0, 2100.0]]
    assert c['n_slots'] == 2 and c['kinds'] == [B.CVAR_DISTANCE] and c['slots'] == [[0, 1]] and c['periodic'] is False and c['globals'] == [0.5]
    assert c['idx'].tolist() == [[0, 1], [2, 0]] and c['params'].tolist() == [[100.0, 200.0]]
    ptr, atoms, weights = c['groups']
    assert ptr.tolist() == [0, 3, 5, 8] and atoms.tolist() == [0, 1, 2, 3, 4, 2, 5, 6] and weights.tolist() == [1.0, 2.0, 3.0, 1.0, 0.0, 2.0, 2.0, 4.0]
    entries = context._engine.entries
    assert [e.term_ids for e in entries] == [[u['id']], [c['id']]] and all(e.term_expr and e.bonded_id is None and not e.terms for e in entries)
    assert entries[0].depends == {'scale'} and entries[1].depends == {'d0'} and list(entries[0].program.code) == u['code']
    # a group's definition ends with the compound force; the existing loops reach it through term_ids
    context._engine._define_group(1)
    assert rec.groups[1][1] == [c['id']]
    # setParameter -> set_globals; a parameter the program does not read changes nothing
    context.setParameter('scale', 0.5)
    assert rec.calls[-1] == ('compound_set_globals', u['id'], [0.5])
    context.setParameter('d0', 0.6)
    assert rec.calls[-1] == ('compound_set_globals', c['id'], [0.6])
    before = len(rec.calls)
    context.setParameter('unused', 4.0)
    assert not [call for call in rec.calls[before:] if call[0].startswith('compound')]
    # updateParametersInContext -> all per-bond values again, and for the centroid class the weights
    ub.setBondParameters(1, [2, 3, 4], [1.7, 320.0, 0.18, 2200.0])
    ub.updateParametersInContext(context)
    call = rec.calls[-1]
    assert call[0] == 'compound_set_params' and call[1] == u['id'] and call[3] == 2 and call[2][:, 1].tolist() == [1.7, 320.0, 0.18, 2200.0]
    cr.setBondParameters(0, [0, 1], [150.0])
    cr.setGroupParameters(1, [3, 4], [1.0, 3.0])
    cr.updateParametersInContext(context)
    assert [call[0] for call in rec.calls[-2:]] == ['compound_set_params', 'compound_set_weights']
    assert rec.calls[-2][2].tolist() == [[150.0, 200.0]] and rec.calls[-1][2].tolist() == [1.0, 2.0, 3.0, 1.0, 3.0, 2.0, 2.0, 4.0]
    # OpenMM's errors: a changed member, a changed count, a group of zero weight
    ub.setBondParameters(1, [2, 3, 5], [1.7, 320.0, 0.18, 2200.0])
    with pytest.raises(openmm.OpenMMException, match='the particles of a bond have changed'):
        ub.updateParametersInContext(context)
    ub.setBondParameters(1, [2, 3, 4], [1.7, 320.0, 0.18, 2200.0])
    ub.addBond([4, 5, 6], [1.7, 320.0, 0.18, 2200.0])
    with pytest.raises(openmm.OpenMMException, match='the number of bonds has changed'):
        ub.updateParametersInContext(context)
    cr.setGroupParameters(1, [3, 5], [1.0, 3.0])
    with pytest.raises(openmm.OpenMMException, match='the particles of a group have changed'):
        cr.updateParametersInContext(context)
    cr.setGroupParameters(1, [3, 4], [1.0, -1.0])
    with pytest.raises(openmm.OpenMMException, match='the weights of group 1 sum to zero'):
        cr.updateParametersInContext(context)
    cr.setGroupParameters(1, [3, 4], [1.0, 3.0])
    cr.addGroup([7])
    with pytest.raises(openmm.OpenMMException, match='the number of groups has changed'):
        cr.updateParametersInContext(context)
    cr.setBondParameters(0, [0, 2], [150.0])
    cr._groups.pop()
    with pytest.raises(openmm.OpenMMException, match='the groups of a bond have changed'):
        cr.updateParametersInContext(context)
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, scale\) of a CustomCompoundBondForce with a generic energy expression'):
        context._engine.energy_derivative('scale')


def test_inner_forces_of_a_collective_variable_force(recorder):
    system = bare_system()
    cv = openmm.CustomCVForce('0.5*K*(d-d0)^2 + a')
    cv.addGlobalParameter('K', 100.0)
    cv.addGlobalParameter('d0', 0.4)
    inner = openmm.CustomCentroidBondForce(2, 'distance(g1,g2)')
    inner.addGroup([0, 1])
    inner.addGroup([2, 3])
    inner.addBond([0, 1])
    cv.addCollectiveVariable('d', inner)
    angle = openmm.CustomCompoundBondForce(3, 'angle(p1,p2,p3)')
    angle.addBond([4, 5, 6])
    cv.addCollectiveVariable('a', angle)
    system.addForce(cv)
    context = context_of(system)
    rec = recorder[-1]
    assert [c['kinds'] for c in rec.compounds] == [[B.CVAR_DISTANCE], [B.CVAR_ANGLE]]
    (create,) = [c for c in rec.calls if c[0] == 'cv_create']
    assert create[2] == [c['id'] for c in rec.compounds]
    (entry,) = context._engine.entries
    assert entry.term_ids == [create[1]] and entry.cv['inner_ids'] == create[2]          # the inner forces are members of no group
    assert 'CustomCompoundBondForce' in E.Engine._CV_INNER_CLASSES and 'CustomCentroidBondForce' in E.Engine._CV_INNER_CLASSES


def test_clean_refusals(recorder):
    def job(rank):
        system = bare_system()
        system.addForce(urey_bradley())
        with pytest.raises(NotImplementedError, match='CustomCompoundBondForce runs on a single rank'):
            context_of(system)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
    for make in (urey_bradley, centroid_restraint):
        system = bare_system()
        force = make()
        force.addTabulatedFunction('tab', openmm.Continuous1DFunction([0.0, 1.0, 2.0], 0.0, 1.0))
        system.addForce(force)
        with pytest.raises(NotImplementedError, match=type(force).__name__ + ': tabulated functions'):
            context_of(system)
        system = bare_system()
        force = make()
        force.addEnergyParameterDerivative('scale')
        system.addForce(force)
        with pytest.raises(NotImplementedError, match=type(force).__name__ + ': addEnergyParameterDerivative'):
            context_of(system)
    for text, message in (('pointdistance(x1,y1,z1,0,0,0)', r'pointdistance\(\.\.\.\) is not supported'),
                          ('distance(p1,p2)*zeta', 'unknown symbol in compound-bond expression: zeta'),
                          ('distance(p1,p2+p1)', 'bare names of particles')):
        system = bare_system()
        system.addForce(openmm.CustomCompoundBondForce(2, text))
        with pytest.raises(atomsmm.InputError, match='CustomCompoundBondForce.*' + message):
            context_of(system)
    system = bare_system()
    system.addForce(openmm.CustomCompoundBondForce(9, 'x9'))
    with pytest.raises(atomsmm.InputError, match=r'1 to 8 particles per bond \(9 given\)'):
        context_of(system)
    system = bare_system()
    force = urey_bradley()
    force.addBond([0, 1, 99], [1.0, 1.0, 1.0, 1.0])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='a particle index is out of range'):
        context_of(system)
    system = bare_system()
    force = centroid_restraint()
    force.addBond([0, 3], [1.0])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='a group index is out of range'):
        context_of(system)
    system = bare_system()
    force = centroid_restraint()
    force.addGroup([1, 2], [1.0, -1.0])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='the weights of group 3 sum to zero'):
        context_of(system)
    system = bare_system()
    force = centroid_restraint()
    force.addGroup([])
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='group 3 is empty'):
        context_of(system)
    # free space: allowed without the flag, refused with it
    for make in (urey_bradley, centroid_restraint):
        system = bare_system(box=False)
        system.addForce(make())
        context_of(system)
        assert recorder[-1].compounds[0]['periodic'] is False and recorder[-1].box is None
        system = bare_system(box=False)
        nb = openmm.NonbondedForce()
        for _ in range(10):
            nb.addParticle(0.0, 0.3, 0.5)
        nb.setNonbondedMethod(nb.NoCutoff)
        system.addForce(nb)
        system.addForce(make(periodic=True))
        with pytest.raises(atomsmm.InputError, match='periodic boundary'):
            context_of(system)


# ------------------------------------------------------------------------------------ 5. the earlier texts compile to the same words
def test_earlier_texts_compile_to_the_parents_words():
    """Every successful compile_pair / compile_term call of tests/test_term_expr_host.py and tests/test_pair_expr_host.py, recorded on
    the commit before compile_per_dof took the hook for calls over names: same code, same constants (bit for bit), same globals."""
    with open(os.path.join(GOLDEN, 'expr_words_parent.json')) as fh:
        recorded = json.load(fh)
    assert len(recorded) >= 30 and {r['function'] for r in recorded} == {'compile_pair', 'compile_term'}
    for r in recorded:
        prog = getattr(X, r['function'])(*r['args'], **r['kwargs'])
        assert [int(w) for w in prog.code] == r['code'], r['args'][0]
        assert [float(c).hex() for c in prog.consts] == r['consts'] and list(prog.globals_) == r['globals'], r['args'][0]
