"""CPU tests of the many-particle force (CustomManyParticleForce over sets of three): the OpenMM-shaped class, the compiler
(expr.compile_many_particle) and its variable table, the permutation table on hand-worked cases, every refusal with its wording --
of the compiler, and of the translation on a recorder over tests/fake_backend.py -- the checker's own inputs
(tests/manyparticle_cases.py: the share of sets its filter keeps), and compile_compound / compile_hbond unchanged: the programs of
the texts of tests/compound_cases.py and tests/hbond_cases.py word for word as the parent commit compiled them."""
import hashlib

import numpy as np
import pytest

import atomsmm_amd as atomsmm
import compound_cases as C
import hbond_cases as H
import manyparticle_cases as M
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import expr as X
from atomsmm_amd import openmm, unit
from fake_backend import RecordingContext

NAMES = {v: k for k, v in X.ALL_OPCODES.items()}


def words(prog):
    return [(NAMES[w & 0xff], w >> 8) for w in prog.code]


# ------------------------------------------------------------------------------------ 1. the class
def test_getters_and_setters():
    force = openmm.CustomManyParticleForce(3, 'k*distance(p1,p2)')
    assert (force.NoCutoff, force.CutoffNonPeriodic, force.CutoffPeriodic) == (0, 1, 2)
    assert (force.SinglePermutation, force.UniqueCentralParticle) == (0, 1)
    assert force.getNumParticlesPerSet() == 3 and openmm.CustomManyParticleForce(5, 'x1').getNumParticlesPerSet() == 5
    assert force.getEnergyFunction() == 'k*distance(p1,p2)' and force.getNonbondedMethod() == force.NoCutoff
    assert force.getPermutationMode() == force.SinglePermutation
    force.setEnergyFunction('g*sig1*distance(p1,p2)')
    assert force.getEnergyFunction() == 'g*sig1*distance(p1,p2)'
    assert force.addPerParticleParameter('sig') == 0 and force.addPerParticleParameter('extra') == 1
    assert force.getNumPerParticleParameters() == 2 and force.getPerParticleParameterName(1) == 'extra'
    force.setPerParticleParameterName(1, 'eps')
    assert force.getPerParticleParameterName(1) == 'eps'
    assert force.addGlobalParameter('g', 2.0 * unit.dimensionless) == 0 and force.getNumGlobalParameters() == 1
    assert force.getGlobalParameterName(0) == 'g' and force.getGlobalParameterDefaultValue(0) == 2.0
    force.setGlobalParameterDefaultValue(0, 3.0)
    force.setGlobalParameterName(0, 'gg')
    assert force.getGlobalParameterDefaultValue(0) == 3.0 and force.getGlobalParameterName(0) == 'gg'
    assert force.addParticle([1.0, 2.0]) == 0 and force.addParticle((3.0, 4.0), 7) == 1 and force.addParticle([5.0, 6.0], type=2) == 2
    assert force.getNumParticles() == 3
    assert force.getParticleParameters(0) == [(1.0, 2.0), 0] and force.getParticleParameters(1) == [(3.0, 4.0), 7]
    force.setParticleParameters(1, [8.0, 9.0], 4)
    assert force.getParticleParameters(1) == [(8.0, 9.0), 4]
    assert force.addExclusion(0, 1) == 0 and force.getNumExclusions() == 1 and force.getExclusionParticles(0) == [0, 1]
    force.setExclusionParticles(0, 1, 2)
    assert force.getExclusionParticles(0) == [1, 2]
    assert force.getTypeFilter(0) == set()
    force.setTypeFilter(1, [4, 2, 2])
    assert force.getTypeFilter(1) == {2, 4} and force.getTypeFilter(2) == set()
    with pytest.raises(openmm.OpenMMException, match='Index out of range'):
        force.setTypeFilter(3, [0])
    assert not force.usesPeriodicBoundaryConditions()
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.43 * unit.nanometers)
    assert force.usesPeriodicBoundaryConditions() and force.getNonbondedMethod() == 2 and force.getCutoffDistance()._value == 0.43
    force.setNonbondedMethod(force.CutoffNonPeriodic)
    assert not force.usesPeriodicBoundaryConditions()
    force.setPermutationMode(force.UniqueCentralParticle)
    assert force.getPermutationMode() == 1
    with pytest.raises(openmm.OpenMMException, match='Illegal value for nonbonded method'):
        force.setNonbondedMethod(3)
    with pytest.raises(openmm.OpenMMException, match='Illegal value for permutation mode'):
        force.setPermutationMode(2)
    assert force.addTabulatedFunction('f', openmm.Continuous1DFunction([0.0, 1.0, 2.0], 0.0, 1.0)) == 0
    assert force.getNumTabulatedFunctions() == 1 and force.getTabulatedFunctionName(0) == 'f'
    force.setForceGroup(4)
    assert force.getForceGroup() == 4 and force.getName() == 'CustomManyParticleForce'


def test_exclusions_from_bonds():
    force = openmm.CustomManyParticleForce(3, 'distance(p1,p2)')
    for _ in range(6):
        force.addParticle()
    force.addExclusion(1, 0)
    force.createExclusionsFromBonds([(0, 1), (1, 2), (2, 3), (4, 5)], 2)
    pairs = sorted(tuple(sorted(force.getExclusionParticles(k))) for k in range(force.getNumExclusions()))
    assert pairs == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (4, 5)]
    with pytest.raises(openmm.OpenMMException, match='Illegal particle index'):
        force.createExclusionsFromBonds([(0, 6)], 1)


# ------------------------------------------------------------------------------------ 2. compile_many_particle
def test_variable_table_and_parameter_slots():
    prog, table = X.compile_many_particle(M.TEXTS['distance']['text'], 3, [], ['k', 'r0'])
    assert table == [('distance', (0, 1))] and prog.globals_ == ['k', 'r0']
    assert words(prog) == [('GLOBAL', 0), ('TERM_VAR', 0), ('GLOBAL', 1), ('SUB', 0), ('POWI', 2), ('MUL', 0)]
    prog, table = X.compile_many_particle(M.TEXTS['stillinger-weber']['text'], 3, [], list(M.TEXTS['stillinger-weber']['globals']))
    assert table == [('angle', (1, 0, 2)), ('distance', (0, 1)), ('distance', (0, 2))]
    prog, table = X.compile_many_particle(M.TEXTS['axilrod-teller']['text'], 3, [], ['C'])
    assert table == [('angle', (0, 1, 2)), ('angle', (1, 2, 0)), ('angle', (2, 0, 1)), ('distance', (0, 1)), ('distance', (1, 2)), ('distance', (0, 2))]
    prog, table = X.compile_many_particle(M.TEXTS['with-dihedral']['text'], 3, [], ['k', 'r0', 'phi'])
    assert ('dihedral', (0, 1, 2, 0)) in table and len(table) == 3
    prog, table = X.compile_many_particle(M.TEXTS['sixteen']['text'], 3, [], list(M.TEXTS['sixteen']['globals']))
    kinds = [k for k, _ in table]
    assert len(table) == 16 and kinds.count('distance') == 5 and kinds.count('angle') == 4 and kinds.count('dihedral') == 1
    assert ('x', (0,)) in table and ('z', (2,)) in table and ('distance', (1, 0)) in table
    # the suffixed copies role by role: sig1 eps1 sig2 eps2 sig3 eps3 = TERM_P 0 .. 5
    assert X.many_particle_parameter_names(3, ['sig', 'eps']) == ['sig1', 'eps1', 'sig2', 'eps2', 'sig3', 'eps3']
    prog, table = X.compile_many_particle('sig1+2*eps1+3*sig2+4*eps2+5*sig3+6*eps3', 3, ['sig', 'eps'], [])
    assert table == [] and [w for w in words(prog) if w[0] == 'TERM_P'] == [('TERM_P', k) for k in range(6)]
    for name, count in M.N_VARIABLES.items():
        case = M.TEXTS[name]
        assert len(X.compile_many_particle(case['text'], 3, case['names'], list(case['globals']))[1]) == count, name
    # the same text as a compound bond of three particles compiles to the same words and the same table
    for name, case in M.TEXTS.items():
        mp = X.compile_many_particle(case['text'], 3, case['names'], list(case['globals']))
        cb = X.compile_compound(case['text'], 3, 'p', M.compound_case(name)['names'], list(case['globals']))
        assert list(mp[0].code) == list(cb[0].code) and mp[0].consts == cb[0].consts and mp[1] == cb[1], name
    # identical calls share a variable; another order of the arguments is another variable
    prog, table = X.compile_many_particle('distance(p1,p2)*distance(p1,p2) + distance(p2,p1) + x1 - x1', 3, [], [])
    assert table == [('distance', (0, 1)), ('distance', (1, 0)), ('x', (0,))]


def test_compiler_refusals():
    with pytest.raises(atomsmm.InputError, match=r'at most 2 per-particle parameters \(3 given'):
        X.compile_many_particle('distance(p1,p2)', 3, list('abc'), [])
    seventeen = M.TEXTS['sixteen']['text'] + ' + y3'
    with pytest.raises(X.ExpressionError, match='many-particle expression: more than 16 distinct geometric variables'):
        X.compile_many_particle(seventeen, 3, [], list(M.TEXTS['sixteen']['globals']))
    for fn in ('pointdistance', 'pointangle', 'pointdihedral'):
        with pytest.raises(X.ExpressionError, match=r'%s\(\.\.\.\) is not supported in a many-particle expression' % fn):
            X.compile_many_particle('%s(0,0,0,1,1,1)' % fn, 3, [], [])
    with pytest.raises(X.ExpressionError, match=r'periodicdistance\(\.\.\.\) is not supported in a many-particle expression'):
        X.compile_many_particle('periodicdistance(0,0,0,1,1,1)', 3, [], [])
    with pytest.raises(X.ExpressionError, match='unsupported function call: table/1'):
        X.compile_many_particle('table(distance(p1,p2))', 3, [], [])
    with pytest.raises(X.ExpressionError, match=r'p4 is none of the particles of a set \(p1 \.\. p3\)'):
        X.compile_many_particle('distance(p1,p4)', 3, [], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in many-particle expression: x4'):
        X.compile_many_particle('x4', 3, [], [])
    with pytest.raises(X.ExpressionError, match=r'the arguments of angle are bare names of particles \(p1 \.\. p3\), not expressions'):
        X.compile_many_particle('angle(p1,p2,2)', 3, [], [])
    with pytest.raises(X.ExpressionError, match='p2 names one of the particles; it stands only as an argument'):
        X.compile_many_particle('p2*distance(p1,p2)', 3, [], [])
    with pytest.raises(X.ExpressionError, match='the per-particle parameter sig is read with the suffix of its particle'):
        X.compile_many_particle('sig*distance(p1,p2)', 3, ['sig'], [])
    with pytest.raises(X.ExpressionError, match='the parameter x1 shadows the coordinate of that name'):
        X.compile_many_particle('x1*distance(p1,p2)', 3, ['x'], [])
    with pytest.raises(X.ExpressionError, match='the per-particle parameter k is declared twice'):
        X.compile_many_particle('k1*distance(p1,p2)', 3, ['k', 'k'], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in many-particle expression: q'):
        X.compile_many_particle('q*distance(p1,p2)', 3, [], [])


# ------------------------------------------------------------------------------------ 3. the permutation table, hand-worked
A_, B_ = 0, 1


def test_permutation_table_without_filters():
    for central in (False, True):
        table = E.many_particle_table([set(), set(), set()], [0], central)
        assert table.tolist() == [[[0]]]
        assert np.array_equal(table, M.permutation_table([set(), set(), set()], [0], central))


def test_permutation_table_two_types_single_mode():
    """Roles (A, B, A).  Tuples in ascending order of the particles: (A, A, B) -> the second permutation (0, 2, 1) puts B in the
    middle; (A, B, A) -> the identity; (B, A, A) -> (1, 0, 2) is the first with A at p1 and B at p2; a tuple without a B, or with
    two, has none."""
    table = E.many_particle_table([{A_}, {B_}, {A_}], [A_, B_], False)
    assert table[A_, A_, B_] == 1 and E.MANY_PERMUTATIONS[1] == (0, 2, 1)
    assert table[A_, B_, A_] == 0
    assert table[B_, A_, A_] == 2 and E.MANY_PERMUTATIONS[2] == (1, 0, 2)
    assert table[A_, A_, A_] == -1 and table[B_, B_, A_] == -1 and table[B_, B_, B_] == -1 and table[A_, B_, B_] == -1
    assert np.array_equal(table, M.permutation_table([{A_}, {B_}, {A_}], [A_, B_], False))
    assert list(map(tuple, E.MANY_PERMUTATIONS)) == M.PERMUTATIONS


def test_permutation_table_two_types_central_mode():
    """The centre stays at p1: only (0, 1, 2) and (0, 2, 1) are candidates.  Roles (A, B, A): the centre must be A, one satellite B."""
    table = E.many_particle_table([{A_}, {B_}, {A_}], [A_, B_], True)
    assert table[A_, B_, A_] == 0 and table[A_, A_, B_] == 1
    assert table[B_, A_, A_] == -1        # (single mode takes this tuple: there the B may move to p2)
    assert table[A_, A_, A_] == -1 and table[A_, B_, B_] == -1
    assert np.array_equal(table, M.permutation_table([{A_}, {B_}, {A_}], [A_, B_], True))


def test_permutation_table_several_admissible_takes_the_first():
    """Roles (any, {A, B}, {B}): tuple (A, B, B) admits (0, 1, 2) and (0, 2, 1) and, in single mode, four more: the first is taken.
    Tuple (B, B, A) admits (0, 1, 2)? p3 = A fails; (0, 2, 1): p2 = A, p3 = B holds -- code 1."""
    filters = [set(), {A_, B_}, {B_}]
    for central in (False, True):
        table = E.many_particle_table(filters, [A_, B_], central)
        assert table[A_, B_, B_] == 0 and table[B_, B_, A_] == 1
        assert table[A_, A_, A_] == -1
        assert np.array_equal(table, M.permutation_table(filters, [A_, B_], central))
    # p3 = B needs (1, 2, 0) or (2, 1, 0) ... in ascending tuple (B, A, A): (1, 2, 0) = (A, A, B) is the first
    assert E.many_particle_table(filters, [A_, B_], False)[B_, A_, A_] == 3 and E.many_particle_table(filters, [A_, B_], True)[B_, A_, A_] == -1
    # types need not be dense: 3 and 7 stand at the dense indices 0 and 1
    assert np.array_equal(E.many_particle_table([{3}, {7}, {3}], [3, 7], False), E.many_particle_table([{A_}, {B_}, {A_}], [A_, B_], False))


def test_the_checker_enumerates_by_the_rule():
    pos = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.4, 0.0], [2.0, 2.0, 2.0]])
    assert M.enumerate_sets(pos, False) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    assert M.enumerate_sets(pos, False, cutoff=0.6) == [(0, 1, 2)]
    assert M.enumerate_sets(pos, False, cutoff=0.45) == []                      # |x1 - x2| = 0.5
    assert M.enumerate_sets(pos, True, cutoff=0.45) == [(0, 1, 2)]              # the satellites' distance is not tested
    assert M.enumerate_sets(pos, True, cutoff=0.6) == [(0, 1, 2), (1, 0, 2), (2, 0, 1)]
    assert M.enumerate_sets(pos, True, [(1, 2)], cutoff=0.6) == []              # an exclusion between satellites removes the set
    assert M.enumerate_sets(pos, False, types=[A_, A_, B_, A_], filters=[{A_}, {B_}, {A_}], cutoff=0.6) == [(0, 2, 1)]
    assert M.enumerate_sets(pos, True, types=[A_, A_, B_, A_], filters=[{A_}, {B_}, {A_}], cutoff=0.6) == [(0, 2, 1), (1, 2, 0)]
    assert M.entries_per_owner([(0, 2, 1), (1, 2, 0)], 4).tolist() == [2, 2, 2, 0]
    # particle 3 at x = 2.85 of a 3 nm box: 0.15 nm from particle 0 by the minimum image only
    pos[3] = [2.85, 0.0, 0.0]
    assert M.enumerate_sets(pos, False, cutoff=0.6) == [(0, 1, 2)]
    assert M.enumerate_sets(pos, False, cutoff=0.6, box=np.full(3, 3.0)) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    assert M.enumerate_sets(pos, False, cutoff=0.44, box=np.full(3, 3.0)) == [(0, 2, 3)]       # |x1 - x3| = 0.45, |x2 - x3| = 0.427


# ------------------------------------------------------------------------------------ 4. the translation, on a recorder
class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.many = []
        self.options = {}

    def set_option(self, name, value):
        self.options[name] = value

    def many_create(self, code, consts, globals_, var_kinds, var_slots, params, types, n_types, perm_table, excl_pairs=None, rc=0.0, periodic=False,
                    central=False):
        fid = self._new()
        self.many.append(dict(id=fid, code=list(code), consts=list(consts), globals=list(globals_), kinds=list(var_kinds),
                              slots=[list(s) for s in var_slots], params=np.array(params), types=np.array(types), n_types=n_types,
                              table=np.array(perm_table), excl=np.array(excl_pairs), rc=rc, periodic=bool(periodic), central=bool(central)))
        return fid

    def many_set_params(self, fid, params, types, n_types, perm_table):
        self.calls.append(('many_set_params', fid, np.array(params), np.array(types), n_types, np.array(perm_table)))

    def many_set_globals(self, fid, globals_):
        self.calls.append(('many_set_globals', fid, list(globals_)))

    def cv_create(self, inner_ids, n_deriv, code, consts, globals_):
        return self._new()


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def bare_system(n=6, box=True):
    system = openmm.System()
    for k in range(n):
        system.addParticle(1.0 + k)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    return system


def context_of(system, integrator=None, properties=None):
    return openmm.Context(system, integrator or openmm.VerletIntegrator(0.001), None, properties)


def fluid(text='scale*eps1*eps2*(distance(p1,p2)-sig3)^2*cos(angle(p2,p1,p3))', method=2, mode=1, n=6, per_set=3):
    force = openmm.CustomManyParticleForce(per_set, text)
    force.addPerParticleParameter('sig')
    force.addPerParticleParameter('eps')
    force.addGlobalParameter('scale', 1.5)
    force.addGlobalParameter('unused', 3.0)
    for k in range(n):
        force.addParticle([0.1 * (k + 1), 1.0 + k], 5 if k % 2 else 2)
    force.addExclusion(0, 1)
    force.addExclusion(4, 2)
    force.setNonbondedMethod(method)
    force.setPermutationMode(mode)
    force.setCutoffDistance(0.43)
    return force


def test_the_force_takes_the_many_particle_route(recorder):
    system = bare_system()
    force = fluid()
    force.setTypeFilter(0, [2])
    force.setForceGroup(3)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    (mp,) = rec.many
    prog, table = X.compile_many_particle(force.getEnergyFunction(), 3, ['sig', 'eps'], ['scale', 'unused'])
    assert mp['code'] == list(prog.code) and mp['consts'] == prog.consts and mp['globals'] == [1.5]
    assert mp['kinds'] == [B.CVAR_DISTANCE, B.CVAR_ANGLE] and mp['slots'] == [[0, 1], [1, 0, 2]] and table == [('distance', (0, 1)), ('angle', (1, 0, 2))]
    assert mp['params'].tolist() == [[0.1 * (k + 1) for k in range(6)], [1.0 + k for k in range(6)]]
    assert mp['types'].tolist() == [0, 1, 0, 1, 0, 1] and mp['n_types'] == 2          # the types 2 and 5 at the dense indices 0 and 1
    assert np.array_equal(mp['table'], M.permutation_table([{2}, set(), set()], [2, 5], True)) and mp['table'][1, 0, 0] == -1
    assert mp['excl'].tolist() == [[0, 1], [4, 2]] and mp['rc'] == 0.43 and mp['periodic'] is True and mp['central'] is True
    (entry,) = context._engine.entries
    assert entry.group == 3 and entry.term_ids == [mp['id']] and entry.term_expr and entry.bonded_id is None
    assert entry.many == dict(id=mp['id'], variables=table, types=2)
    # a global, then the parameters, the types and the filters again
    context.setParameter('scale', 2.0)
    assert rec.calls[-1] == ('many_set_globals', mp['id'], [2.0])
    before = len(rec.calls)
    context.setParameter('unused', 1.0)
    assert len(rec.calls) == before
    force.setParticleParameters(1, [9.0, 8.0], 7)
    force.setTypeFilter(1, [7])
    force.updateParametersInContext(context)
    name, fid, par, types, n_types, perm = rec.calls[-1]
    assert (name, fid, n_types) == ('many_set_params', mp['id'], 3) and types.tolist() == [0, 2, 0, 1, 0, 1]     # ... of 2, 5, 7
    assert par[:, 1].tolist() == [9.0, 8.0] and np.array_equal(perm, M.permutation_table([{2}, {7}, set()], [2, 5, 7], True))
    force.addExclusion(0, 3)
    with pytest.raises(openmm.OpenMMException, match='updateParametersInContext: the exclusions have changed'):
        force.updateParametersInContext(context)
    force.setExclusionParticles(2, 0, 1)
    force._exclusions.pop()
    force.addParticle([1.0, 1.0])
    with pytest.raises(openmm.OpenMMException, match='updateParametersInContext: the number of particles has changed'):
        force.updateParametersInContext(context)


def test_methods_modes_and_options_reach_the_backend(recorder):
    for method, rc, periodic in ((0, 0.0, False), (1, 0.43, False), (2, 0.43, True)):
        for mode in (0, 1):
            system = bare_system()
            system.addForce(fluid(method=method, mode=mode))
            context_of(system)
            got = recorder[-1].many[0]
            assert (got['rc'], got['periodic'], got['central']) == (rc, periodic, bool(mode))
    system = bare_system(box=False)
    system.addForce(fluid(method=0))
    assert context_of(system, properties={'Option.many_capacity': 64})._engine.free_space and recorder[-1].many[0]['rc'] == 0.0
    assert recorder[-1].options['many_capacity'] == 64.0


def test_refusals_when_the_context_is_created(recorder, monkeypatch):
    def refused(force, exc, match, system=None, integrator=None):
        system = system or bare_system()
        system.addForce(force)
        with pytest.raises(exc, match=match):
            context_of(system, integrator)

    for per_set in (2, 4):
        refused(fluid(per_set=per_set), NotImplementedError, r'CustomManyParticleForce: sets of %d particles are not supported \(the many-particle kernel '
                                                               'enumerates sets of three' % per_set)
    # the compiler's refusals arrive with the class's name
    refused(fluid('pointdistance(0,0,0,1,1,1)'), atomsmm.InputError, r'CustomManyParticleForce: not an energy expression.*pointdistance\(\.\.\.\) is not supported')
    refused(fluid('periodicdistance(0,0,0,1,1,1)'), atomsmm.InputError, r'CustomManyParticleForce: not an energy expression.*periodicdistance\(\.\.\.\) is not supported')
    refused(fluid('sig*distance(p1,p2)'), atomsmm.InputError, 'CustomManyParticleForce: not an energy expression the many-particle kernel can run: .*read with the suffix')
    force = fluid()
    force.addPerParticleParameter('third')
    refused(force, atomsmm.InputError, 'at most 2 per-particle parameters')
    force = fluid()
    force.addTabulatedFunction('f', openmm.Continuous1DFunction([0.0, 1.0, 2.0], 0.0, 1.0))
    refused(force, NotImplementedError, 'CustomManyParticleForce: tabulated functions in the energy expression are not supported')
    # counts, indices, types
    refused(fluid(n=5), openmm.OpenMMException, 'CustomManyParticleForce: the force has 5 particles, the System 6')
    force = fluid()
    force.addExclusion(6, 0)
    refused(force, openmm.OpenMMException, 'CustomManyParticleForce: an exclusion names a particle that does not exist')
    force = fluid()
    force.setParticleParameters(2, [1.0], 2)
    refused(force, openmm.OpenMMException, 'CustomManyParticleForce: every particle needs 2 parameters')
    force = fluid(n=17)
    for k in range(17):
        force.setParticleParameters(k, [0.1, 1.0], 10 * k)
    refused(force, atomsmm.InputError, r'CustomManyParticleForce: 17 distinct particle types \(limit 16\)', system=bare_system(17))
    refused(fluid(n=2049, method=0), atomsmm.InputError, r'CustomManyParticleForce: 2049 particles under NoCutoff \(limit 2048', system=bare_system(2049))
    force = fluid()
    force.setCutoffDistance(0.0)
    refused(force, atomsmm.InputError, 'CustomManyParticleForce: the cutoff distance must be above zero')
    # CutoffPeriodic in a System in free space
    nb = openmm.NonbondedForce()
    for _ in range(6):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.NoCutoff)
    system = bare_system()
    system.addForce(nb)
    refused(fluid(method=2), atomsmm.InputError, 'a CustomManyParticleForce that uses periodic boundary', system=system)
    # as a collective variable
    cv = openmm.CustomCVForce('2*mp')
    cv.addCollectiveVariable('mp', fluid())
    refused(cv, NotImplementedError, 'CustomManyParticleForce')
    # deriv(energy, ...) through it
    integrator = openmm.CustomIntegrator(0.001)
    integrator.addGlobalVariable('g', 0.0)
    integrator.addComputeGlobal('g', 'deriv(energy, scale)')
    refused(fluid(), NotImplementedError, r'deriv\(energy, \.\.\.\) through a CustomManyParticleForce is not supported', integrator=integrator)
    # the virial computers
    system = bare_system()
    system.addForce(fluid())
    with pytest.raises(NotImplementedError, match='ComputingSystem / PressureComputer: the virial of a CustomManyParticleForce is not supported'):
        atomsmm.ComputingSystem(system)


def test_more_than_32768_particles_are_refused(recorder):
    n = 32769
    system = bare_system(n)
    force = openmm.CustomManyParticleForce(3, 'distance(p1,p2)')
    for _ in range(n):
        force.addParticle()
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.4)
    system.addForce(force)
    with pytest.raises(atomsmm.InputError, match=r'CustomManyParticleForce: 32769 particles \(limit 32768\)'):
        context_of(system)


def test_several_ranks_are_refused(recorder, monkeypatch):
    class TwoRanks:
        world = 2
    system = bare_system()
    system.addForce(fluid())
    monkeypatch.setattr(E.LocalWorld, 'current', staticmethod(lambda: (TwoRanks(), 0)))
    with pytest.raises(atomsmm.InputError, match='a CustomManyParticleForce runs on a single rank'):
        context_of(system)


# ------------------------------------------------------------------------------------ 5. the checker's own inputs
@pytest.mark.parametrize('periodic', (False, True), ids=('free', 'periodic'))
@pytest.mark.parametrize('central', (False, True), ids=('single', 'central'))
@pytest.mark.parametrize('n', sorted(M.SMALL_SEEDS))
@pytest.mark.parametrize('name', ('distance', 'three', 'sixteen', 'with-dihedral'))
def test_the_filter_keeps_95_percent(name, n, central, periodic):
    """The seeds of the reference comparisons of tests/test_gpu_manyparticle.py: every case has a set, and the filter keeps at least
    95 % of them, with and without the cutoff."""
    pos = M.small_layout(n, periodic)
    box = np.full(3, M.SMALL_EDGE) if periodic else None
    par = M.parameters(name, n, 5)
    for cutoff in ((M.SMALL_CUTOFF,) if periodic else (None, M.SMALL_CUTOFF)):
        assert cutoff is None or M.margin_ok(pos, cutoff, box)
        sets = M.enumerate_sets(pos, central, (), cutoff, box)
        kept = [s for s in sets if M.usable(name, pos, s, M.set_parameters(par, s), cutoff, box, central)]
        print('%s, n = %d, %s, cutoff %s, box %s: %d of %d sets usable' % (name, n, 'central' if central else 'single', cutoff, box is not None, len(kept), len(sets)))
        assert len(sets) >= 1 and len(kept) >= M.MIN_KEPT * len(sets)
        if cutoff is None:
            assert len(sets) == (3 if central else 1) * n * (n - 1) * (n - 2) // 6
    if periodic and n == 6:       # some of it only by the minimum image
        assert len(M.enumerate_sets(pos, central, (), M.SMALL_CUTOFF, box)) > len(M.enumerate_sets(pos, central, (), M.SMALL_CUTOFF, None))


def test_the_layouts_of_the_gpu_tests():
    rc = 0.5
    pos = M.rows_layout(rc)
    assert M.margin_ok(pos, rc)
    assert sorted(len(r) for r in M.neighbours(pos, (), rc)) == [1] * 2 + [2] * 3 + [12] * 13
    for m, removed, target in ((12, 3, 63), (12, 2, 64), (12, 1, 65), (17, 8, 128), (17, 7, 129)):
        pos = M.cluster_layout(m, rc, 40 + m)
        excl = [(2 * k + 1, 2 * k + 2) for k in range(removed)]
        assert M.margin_ok(pos, rc) and all(len(r) == m for r in M.neighbours(pos, (), rc))
        assert M.entries_per_owner(M.enumerate_sets(pos, False, excl, rc), m + 1)[0] == target
    for m in (64, 65):
        assert all(len(r) == m for r in M.neighbours(M.cluster_layout(m, 1.2, 90 + m), (), 1.2))


# ------------------------------------------------------------------------------------ 6. the other compilers are unchanged
def digest(prog, table):
    return hashlib.sha256(repr((list(prog.code), [float(c).hex() for c in prog.consts], list(prog.globals_), table)).encode()).hexdigest()[:16]


def test_compile_compound_and_compile_hbond_emit_the_parents_words():
    """The digests of (words, constants, globals, variable table) as the parent commit compiled them."""
    got = {}
    for name, case in C.TEXTS.items():
        prefix = 'g' if name.startswith('centre') else 'p'
        got['compound:' + name] = digest(*X.compile_compound(case['text'], case['n'], prefix, case['names'], list(case['globals'])))
    for name, case in H.TEXTS.items():
        got['hbond:' + name] = digest(*X.compile_hbond(case['text'], case['dnames'], case['anames'], list(case['globals'])))
    print(got)
    assert got == PARENT_DIGESTS


PARENT_DIGESTS = {
    'compound:centre-angle': 'c2b23a6ce17e3bea', 'compound:centre-distance': 'b49df5c2b9ac735f', 'compound:five': '36c1f75dc9e1f12d',
    'compound:harmonic-angle': 'fb3a377513809cc2', 'compound:harmonic-bond': '8e51cc661159ef8e', 'compound:periodic-torsion': '1b206eb552d49fca',
    'compound:sixteen': '4e4193efe8168dc9', 'compound:stretch-bend': '5d136ae28f563db3', 'compound:torsion-14': '5ffe1dc262f55720',
    'compound:urey-bradley': 'aefb2b2fea3f0a2f', 'hbond:distance': '2be0f94feacccb3b', 'hbond:distance-angle': '0d0e7f4e2e382f0f',
    'hbond:parameters': '115e6f7a044bc9aa', 'hbond:sixteen': 'd7f50fa2c1a72ff1', 'hbond:three': '749314e942334bdd',
    'hbond:with-dihedral': '967d0a56dd494c84',
}
