"""CPU tests of the hydrogen-bond force (CustomHbondForce with any energy text): the OpenMM-shaped class, the compiler
(expr.compile_hbond) and its variable table, every refusal with its wording -- of the compiler, and of the translation on a recorder
over tests/fake_backend.py -- the checker's own inputs (tests/hbond_cases.py: the share of surviving pairs its filter keeps), and
compile_compound unchanged: the programs of the texts of tests/compound_cases.py word for word as the parent commit compiled them."""
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import compound_cases as C
import hbond_cases as H
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
    force = openmm.CustomHbondForce('k*distance(d1,a1)')
    assert (force.NoCutoff, force.CutoffNonPeriodic, force.CutoffPeriodic) == (0, 1, 2)
    assert force.getEnergyFunction() == 'k*distance(d1,a1)' and force.getNonbondedMethod() == force.NoCutoff
    force.setEnergyFunction('kd*ka*g*distance(d1,a1)')
    assert force.getEnergyFunction() == 'kd*ka*g*distance(d1,a1)'
    assert force.addPerDonorParameter('kd') == 0 and force.addPerDonorParameter('extra') == 1 and force.addPerAcceptorParameter('ka') == 0
    assert force.getNumPerDonorParameters() == 2 and force.getNumPerAcceptorParameters() == 1
    assert force.getPerDonorParameterName(1) == 'extra' and force.getPerAcceptorParameterName(0) == 'ka'
    force.setPerDonorParameterName(1, 'other')
    force.setPerAcceptorParameterName(0, 'kacc')
    assert force.getPerDonorParameterName(1) == 'other' and force.getPerAcceptorParameterName(0) == 'kacc'
    assert force.addGlobalParameter('g', 2.0 * unit.dimensionless) == 0 and force.getNumGlobalParameters() == 1
    assert force.getGlobalParameterName(0) == 'g' and force.getGlobalParameterDefaultValue(0) == 2.0
    force.setGlobalParameterDefaultValue(0, 3.0)
    force.setGlobalParameterName(0, 'gg')
    assert force.getGlobalParameterDefaultValue(0) == 3.0 and force.getGlobalParameterName(0) == 'gg'
    assert force.addDonor(1, 0, -1, [1.0, 2.0]) == 0 and force.addDonor(2, 0, -1, (3.0, 4.0)) == 1
    assert force.addAcceptor(5, -1, -1, [7.0]) == 0
    assert force.getNumDonors() == 2 and force.getNumAcceptors() == 1
    assert force.getDonorParameters(1) == [2, 0, -1, (3.0, 4.0)] and force.getAcceptorParameters(0) == [5, -1, -1, (7.0,)]
    force.setDonorParameters(1, 2, 0, 3, [5.0, 6.0])
    force.setAcceptorParameters(0, 5, 4, -1, [8.0])
    assert force.getDonorParameters(1) == [2, 0, 3, (5.0, 6.0)] and force.getAcceptorParameters(0) == [5, 4, -1, (8.0,)]
    assert force.addExclusion(0, 0) == 0 and force.getNumExclusions() == 1 and force.getExclusionParticles(0) == [0, 0]
    force.setExclusionParticles(0, 1, 0)
    assert force.getExclusionParticles(0) == [1, 0]
    assert not force.usesPeriodicBoundaryConditions()
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.35 * unit.nanometers)
    assert force.usesPeriodicBoundaryConditions() and force.getNonbondedMethod() == 2 and force.getCutoffDistance()._value == 0.35
    force.setNonbondedMethod(force.CutoffNonPeriodic)
    assert not force.usesPeriodicBoundaryConditions()
    with pytest.raises(openmm.OpenMMException, match='Illegal value for nonbonded method'):
        force.setNonbondedMethod(3)
    force.setForceGroup(4)
    assert force.getForceGroup() == 4 and force.getName() == 'CustomHbondForce'


# ------------------------------------------------------------------------------------ 2. compile_hbond
def test_variable_table_of_the_case_texts():
    prog, table = X.compile_hbond(H.TEXTS['distance']['text'], [], [], ['k', 'r0'])
    assert table == [('distance', (0, 3))] and prog.globals_ == ['k', 'r0']
    assert words(prog) == [('GLOBAL', 0), ('TERM_VAR', 0), ('GLOBAL', 1), ('SUB', 0), ('POWI', 2), ('MUL', 0)]
    prog, table = X.compile_hbond(H.TEXTS['three']['text'], [], [], ['k', 'r0', 'phi'])
    assert table == [('distance', (0, 3)), ('angle', (1, 0, 3)), ('dihedral', (1, 0, 3, 4))]
    case = H.TEXTS['sixteen']
    prog, table = X.compile_hbond(case['text'], case['dnames'], case['anames'], list(case['globals']))
    assert len(table) == 16 and [k for k, _ in table].count('distance') == 8 and [k for k, _ in table].count('angle') == 5
    assert table[0] == ('distance', (0, 3)) and ('dihedral', (2, 1, 0, 3)) in table and ('distance', (1, 0)) in table
    # per-donor parameters first, the per-acceptor ones behind them
    assert {w for w in words(prog) if w[0] == 'TERM_P'} == {('TERM_P', k) for k in range(4)}
    prog, table = X.compile_hbond('kd*ka', ['kd'], ['ka'], [])
    assert table == [] and words(prog) == [('TERM_P', 0), ('TERM_P', 1), ('MUL', 0)]
    for name, count in H.N_VARIABLES.items():
        case = H.TEXTS[name]
        assert len(X.compile_hbond(case['text'], case['dnames'], case['anames'], list(case['globals']))[1]) == count, name
    # the same text over p1 .. p6 compiles to the same words and the same table
    for name, case in H.TEXTS.items():
        hb = X.compile_hbond(case['text'], case['dnames'], case['anames'], list(case['globals']))
        cb = X.compile_compound(H.compound_text(case['text']), 6, 'p', case['dnames'] + case['anames'], list(case['globals']))
        assert list(hb[0].code) == list(cb[0].code) and hb[0].consts == cb[0].consts and hb[1] == cb[1], name


def test_identical_calls_share_a_variable():
    prog, table = X.compile_hbond('distance(d1,a1)*distance(d1,a1) + distance(a1,d1) + angle(d2,d1,a1) - angle(d2, d1, a1); unused = distance(d3,a3)',
                                  [], [], [])
    assert table == [('distance', (0, 3)), ('distance', (3, 0)), ('angle', (1, 0, 3))]
    assert [w for w in words(prog) if w[0] == 'TERM_VAR'] == [('TERM_VAR', k) for k in (0, 0, 1, 2, 2)]


def test_compiler_refusals():
    with pytest.raises(atomsmm.InputError, match=r'at most 8 per-donor and per-acceptor parameters together \(5 \+ 4 given\)'):
        X.compile_hbond('distance(d1,a1)', list('abcde'), list('fghi'), [])
    seventeen = '+'.join('distance(%s,%s)' % (a, b) for a in ('d1', 'd2', 'd3', 'a1', 'a2', 'a3') for b in ('d1', 'd2', 'd3', 'a1', 'a2', 'a3') if a != b)
    with pytest.raises(X.ExpressionError, match='hydrogen-bond expression: more than 16 distinct geometric variables'):
        X.compile_hbond(seventeen, [], [], [])
    with pytest.raises(X.ExpressionError, match='the raw coordinate x1 is not supported'):
        X.compile_hbond('x1*distance(d1,a1)', [], [], [])
    with pytest.raises(X.ExpressionError, match='the raw coordinate z4 is not supported'):
        X.compile_hbond('distance(d1,a1) - z4', [], [], [])
    assert X.compile_hbond('x1*distance(d1,a1)', ['x1'], [], [])[1] == [('distance', (0, 3))]        # (a parameter may bear that name)
    for fn in ('pointdistance', 'pointangle', 'pointdihedral'):
        with pytest.raises(X.ExpressionError, match=r'%s\(\.\.\.\) is not supported in a hydrogen-bond expression' % fn):
            X.compile_hbond('%s(0,0,0,1,1,1)' % fn, [], [], [])
    with pytest.raises(X.ExpressionError, match=r'periodicdistance\(\.\.\.\) is not supported in a hydrogen-bond expression'):
        X.compile_hbond('periodicdistance(0,0,0,1,1,1)', [], [], [])
    with pytest.raises(X.ExpressionError, match='unsupported function call: table/1'):
        X.compile_hbond('table(distance(d1,a1))', [], [], [])
    with pytest.raises(X.ExpressionError, match=r'p1 is none of the particles of a donor-acceptor pair \(d1 d2 d3 a1 a2 a3\)'):
        X.compile_hbond('distance(d1,p1)', [], [], [])
    with pytest.raises(X.ExpressionError, match=r'the arguments of angle are bare names of particles \(d1 d2 d3 a1 a2 a3\), not expressions'):
        X.compile_hbond('angle(d1,a1,2)', [], [], [])
    with pytest.raises(X.ExpressionError, match='d2 names one of the particles; it stands only as an argument'):
        X.compile_hbond('d2*distance(d1,a1)', [], [], [])
    with pytest.raises(X.ExpressionError, match='dihedral takes 4 particles \\(3 given\\)'):
        X.compile_hbond('dihedral(d1,a1,a2)', [], [], [])
    with pytest.raises(X.ExpressionError, match='the parameter a1 shadows the particle of that name'):
        X.compile_hbond('a1*distance(d1,a1)', [], ['a1'], [])
    with pytest.raises(X.ExpressionError, match='the parameter k is declared twice among the per-donor and per-acceptor parameters'):
        X.compile_hbond('k*distance(d1,a1)', ['k'], ['k'], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in hydrogen-bond expression: q'):
        X.compile_hbond('q*distance(d1,a1)', [], [], [])


# ------------------------------------------------------------------------------------ 3. the translation, on a recorder
class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.hbonds = []

    def hbond_create(self, code, consts, globals_, var_kinds, var_slots, donors, acceptors, donor_params, acceptor_params, excl_pairs=None, rc=0.0,
                     periodic=False):
        fid = self._new()
        self.hbonds.append(dict(id=fid, code=list(code), consts=list(consts), globals=list(globals_), kinds=list(var_kinds),
                                slots=[list(s) for s in var_slots], donors=np.array(donors), acceptors=np.array(acceptors),
                                dpar=np.array(donor_params), apar=np.array(acceptor_params), excl=np.array(excl_pairs), rc=rc, periodic=bool(periodic)))
        return fid

    def hbond_set_params(self, fid, donor_params, n_donors, acceptor_params, n_acceptors):
        self.calls.append(('hbond_set_params', fid, np.array(donor_params), n_donors, np.array(acceptor_params), n_acceptors))

    def hbond_set_globals(self, fid, globals_):
        self.calls.append(('hbond_set_globals', fid, list(globals_)))

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


def bare_system(n=9, box=True):
    system = openmm.System()
    for k in range(n):
        system.addParticle(1.0 + k)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    return system


def context_of(system, integrator=None):
    return openmm.Context(system, integrator or openmm.VerletIntegrator(0.001))


def water_like(text='scale*kd*ka*(distance(d1,a1)-r0)^2*cos(angle(d2,d1,a1))', method=2):
    force = openmm.CustomHbondForce(text)
    force.addPerDonorParameter('kd')
    force.addPerAcceptorParameter('ka')
    force.addPerAcceptorParameter('r0')
    force.addGlobalParameter('scale', 1.5)
    force.addGlobalParameter('unused', 3.0)
    for m in range(3):
        force.addDonor(3 * m + 1, 3 * m, -1, [1.0 + m])
        force.addDonor(3 * m + 2, 3 * m, -1, [1.5 + m])
        force.addAcceptor(3 * m, 3 * m + 1, 3 * m + 2, [2.0 + m, 0.3])
        force.addExclusion(2 * m, m)
        force.addExclusion(2 * m + 1, m)
    force.setNonbondedMethod(method)
    force.setCutoffDistance(0.35)
    return force


def test_the_force_takes_the_hbond_route(recorder):
    system = bare_system()
    force = water_like()
    force.setForceGroup(3)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    (hb,) = rec.hbonds
    prog, table = X.compile_hbond(force.getEnergyFunction(), ['kd'], ['ka', 'r0'], ['scale', 'unused'])
    assert hb['code'] == list(prog.code) and hb['consts'] == prog.consts and hb['globals'] == [1.5]
    assert hb['kinds'] == [B.CVAR_DISTANCE, B.CVAR_ANGLE] and hb['slots'] == [[0, 3], [1, 0, 3]] and table == [('distance', (0, 3)), ('angle', (1, 0, 3))]
    assert hb['donors'].tolist() == [[1, 0, -1], [2, 0, -1], [4, 3, -1], [5, 3, -1], [7, 6, -1], [8, 6, -1]]
    assert hb['acceptors'].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert hb['dpar'].tolist() == [[1.0, 1.5, 2.0, 2.5, 3.0, 3.5]] and hb['apar'].tolist() == [[2.0, 3.0, 4.0], [0.3, 0.3, 0.3]]
    assert hb['excl'].tolist() == [[0, 0], [1, 0], [2, 1], [3, 1], [4, 2], [5, 2]] and hb['rc'] == 0.35 and hb['periodic'] is True
    (entry,) = context._engine.entries
    assert entry.group == 3 and entry.term_ids == [hb['id']] and entry.term_expr and entry.bonded_id is None
    assert entry.hbond == dict(id=hb['id'], variables=table)
    # a global, then the parameters again
    context.setParameter('scale', 2.0)
    assert rec.calls[-1] == ('hbond_set_globals', hb['id'], [2.0])
    before = len(rec.calls)
    context.setParameter('unused', 1.0)
    assert len(rec.calls) == before
    force.setDonorParameters(1, 2, 0, -1, [9.0])
    force.setAcceptorParameters(2, 6, 7, 8, [5.0, 0.31])
    force.updateParametersInContext(context)
    name, fid, dpar, nd, apar, na = rec.calls[-1]
    assert (name, fid, nd, na) == ('hbond_set_params', hb['id'], 6, 3)
    assert dpar.tolist() == [[1.0, 9.0, 2.0, 2.5, 3.0, 3.5]] and apar.tolist() == [[2.0, 3.0, 5.0], [0.3, 0.3, 0.31]]
    force.setDonorParameters(1, 2, 1, -1, [9.0])
    with pytest.raises(openmm.OpenMMException, match='updateParametersInContext: the particles of a donor or an acceptor have changed'):
        force.updateParametersInContext(context)
    force.setDonorParameters(1, 2, 0, -1, [9.0])
    force.addExclusion(0, 1)
    with pytest.raises(openmm.OpenMMException, match='updateParametersInContext: the exclusions have changed'):
        force.updateParametersInContext(context)


def test_methods_and_cutoffs_reach_the_backend(recorder):
    for method, rc, periodic in ((0, 0.0, False), (1, 0.35, False), (2, 0.35, True)):
        system = bare_system()
        system.addForce(water_like(method=method))
        context_of(system)
        assert (recorder[-1].hbonds[0]['rc'], recorder[-1].hbonds[0]['periodic']) == (rc, periodic)
    system = bare_system(box=False)
    system.addForce(water_like(method=0))
    assert context_of(system)._engine.free_space and recorder[-1].hbonds[0]['rc'] == 0.0


def test_refusals_when_the_context_is_created(recorder, monkeypatch):
    def refused(force, exc, match, system=None, integrator=None):
        system = system or bare_system()
        system.addForce(force)
        with pytest.raises(exc, match=match):
            context_of(system, integrator)

    # a text that names a slot which some donor or acceptor leaves at -1
    refused(water_like('distance(d1,a1)*angle(d3,d1,a1)'), atomsmm.InputError, 'CustomHbondForce: the energy expression names d3, which donor 0 leaves at -1')
    force = water_like('distance(d1,a1)*angle(d1,a1,a3)')
    force.setAcceptorParameters(1, 3, 4, -1, [1.0, 0.3])
    refused(force, atomsmm.InputError, 'CustomHbondForce: the energy expression names a3, which acceptor 1 leaves at -1')
    # the compiler's refusals arrive with the class's name
    refused(water_like('x1*distance(d1,a1)'), atomsmm.InputError,
            'CustomHbondForce: not an energy expression the hydrogen-bond kernel can run: .*the raw coordinate x1 is not supported')
    refused(water_like('pointdistance(0,0,0,1,1,1)'), atomsmm.InputError, r'CustomHbondForce: not an energy expression.*pointdistance\(\.\.\.\) is not supported')
    force = water_like()
    force.addTabulatedFunction('f', openmm.Continuous1DFunction([0.0, 1.0, 2.0], 0.0, 1.0))
    refused(force, NotImplementedError, 'CustomHbondForce: tabulated functions in the energy expression are not supported')
    # indices
    force = water_like()
    force.addDonor(9, 0, -1, [1.0])
    refused(force, openmm.OpenMMException, 'CustomHbondForce: a particle index of donor 6 is out of range')
    force = water_like()
    force.addAcceptor(-1, 0, 1, [1.0, 0.3])
    refused(force, openmm.OpenMMException, 'CustomHbondForce: a particle index of acceptor 3 is out of range')
    force = water_like()
    force.addExclusion(6, 0)
    refused(force, openmm.OpenMMException, 'CustomHbondForce: an exclusion names a donor or an acceptor that does not exist')
    force = water_like()
    force.addDonor(1, 0, -1, [])
    refused(force, openmm.OpenMMException, 'CustomHbondForce: every donor needs 1 parameters')
    # CutoffPeriodic in a System in free space
    nb = openmm.NonbondedForce()
    for _ in range(9):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.NoCutoff)
    system = bare_system()
    system.addForce(nb)
    refused(water_like(method=2), atomsmm.InputError, 'a CustomHbondForce that uses periodic boundary conditions', system=system)
    # as a collective variable
    cv = openmm.CustomCVForce('2*hb')
    cv.addCollectiveVariable('hb', water_like())
    refused(cv, NotImplementedError, 'CustomHbondForce')
    # deriv(energy, ...) through it
    integrator = openmm.CustomIntegrator(0.001)
    integrator.addGlobalVariable('g', 0.0)
    integrator.addComputeGlobal('g', 'deriv(energy, scale)')
    refused(water_like(), NotImplementedError, r'deriv\(energy, \.\.\.\) through a CustomHbondForce is not supported', integrator=integrator)
    # the virial computers
    system = bare_system()
    system.addForce(water_like())
    with pytest.raises(NotImplementedError, match='ComputingSystem / PressureComputer: the virial of a CustomHbondForce is not supported'):
        atomsmm.ComputingSystem(system)


def test_several_ranks_are_refused(recorder, monkeypatch):
    class TwoRanks:
        world = 2
    system = bare_system()
    system.addForce(water_like())
    monkeypatch.setattr(E.LocalWorld, 'current', staticmethod(lambda: (TwoRanks(), 0)))
    with pytest.raises(atomsmm.InputError, match='a CustomHbondForce runs on a single rank'):
        context_of(system)


# ------------------------------------------------------------------------------------ 4. the checker's own inputs
LAYOUT_SEEDS = {(1, 1): 3, (1, 65): 11}


@pytest.mark.parametrize('shape', sorted(LAYOUT_SEEDS))
@pytest.mark.parametrize('name', ('distance', 'three', 'sixteen'))
def test_the_filter_keeps_95_percent(name, shape):
    """The seeds of the reference comparisons of tests/test_gpu_hbond.py: the filter keeps at least 95 % of the pairs."""
    pos, donors, acceptors = H.layout(shape[0], shape[1], 2.5, LAYOUT_SEEDS[shape])
    dpar, apar = H.parameters(name, shape[0], 'd', 5), H.parameters(name, shape[1], 'a', 5)
    pairs = H.survivors(pos, donors, acceptors)
    assert len(pairs) == shape[0] * shape[1]
    kept = [p for p in pairs if H.usable(name, pos, donors, acceptors, p, list(dpar[p[0]]) + list(apar[p[1]]))]
    print('%s, %d x %d: %d of %d pairs usable' % (name, shape[0], shape[1], len(kept), len(pairs)))
    assert len(kept) >= H.MIN_KEPT * len(pairs)


def test_survivors_and_rewriting():
    assert H.compound_text('distance(d1,a1)*angle(d2,d1,a3) + kd1') == 'distance(p1,p4)*angle(p2,p1,p6) + kd1'
    pos, donors, acceptors, excl = H.water_layout(27, 0.95, 4)
    box = np.full(3, 0.95)
    assert donors.shape == (54, 3) and acceptors.shape == (27, 3) and len(excl) == 54
    inside = H.survivors(pos, donors, acceptors, excl, 0.35, box)
    raw = H.survivors(pos, donors, acceptors, excl, 0.35, None)
    assert 0 < len(raw) < len(inside) < 54 * 27 - 54       # some pairs straddle a face
    assert not set(inside) & set(excl) and set(raw) <= set(inside)
    assert len(H.survivors(pos, donors, acceptors)) == 54 * 27
    assert H.members_of(donors, acceptors, (3, 2)) == [5, 3, 5, 6, 7, 8]
    assert H.named_slots('distance') == [0, 3] and H.named_slots('three') == [0, 1, 3, 4] and H.named_slots('sixteen') == [0, 1, 2, 3, 4, 5]
    # the reference of one pair against the closed form
    e, f, kept, looked = H.reference('distance', pos, donors, acceptors, np.zeros((54, 0)), np.zeros((27, 0)), [inside[0]], box)
    d = pos[donors[inside[0][0], 0]] - pos[acceptors[inside[0][1], 0]]
    d -= box * np.rint(d / box)
    r = np.linalg.norm(d)
    assert (len(kept), looked) == (1, 1) and e == pytest.approx(40.0 * (r - 0.3) ** 2, rel=1e-13)
    assert np.allclose(f[donors[inside[0][0], 0]], -80.0 * (r - 0.3) * d / r, rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------ 5. compile_compound unchanged
def test_compile_compound_emits_the_parents_words():
    """The texts of tests/compound_cases.py: code words, constants (bit for bit), globals and variable tables as the commit before
    compile_compound and compile_hbond came to share their body compiled them (captured there, written out here)."""
    assert set(PARENT) == set(C.TEXTS)
    for name, (code, consts, globals_, table) in PARENT.items():
        case = C.TEXTS[name]
        prog, variables = X.compile_compound(case['text'], case['n'], 'g' if name.startswith('centre') else 'p', case['names'], list(case['globals']))
        assert [int(w) for w in prog.code] == code, name
        assert [float(c).hex() for c in prog.consts] == consts and list(prog.globals_) == globals_ and variables == table, name
    # ... and its messages
    with pytest.raises(X.ExpressionError, match=r'compound-bond expression: p9 is none of the particles of a bond \(p1 \.\. p2\)'):
        X.compile_compound('distance(p1,p9)', 2, 'p', [], [])
    with pytest.raises(X.ExpressionError, match=r'compound-bond expression: the arguments of distance are bare names of groups \(g1 \.\. g3\), not expressions'):
        X.compile_compound('distance(g1,1)', 3, 'g', [], [])
    with pytest.raises(X.ExpressionError, match='compound-bond expression: the parameter x1 shadows the coordinate of that name'):
        X.compile_compound('x1*distance(p1,p2)', 2, 'p', ['x1'], [])
    with pytest.raises(X.ExpressionError, match='unknown symbol in compound-bond expression: q'):
        X.compile_compound('q*distance(p1,p2)', 2, 'p', [], [])


PARENT = {'centre-angle': ([54, 0, 53, 310, 11, 24, 11, 12, 1, 309, 565, 11, 528, 12, 10], ['0x1.0000000000000p+0'], ['kx'],
                  [('angle', (0, 1, 2)), ('x', (0,)), ('x', (2,))]),
 'centre-distance': ([0, 54, 12, 53, 310, 11, 528, 12], ['0x1.0000000000000p-1'], [], [('distance', (0, 1))]),
 'five': ([1, 54, 53, 310, 11, 528, 12, 566, 309, 24, 12, 10, 822, 565, 1078, 11, 528, 12, 10, 1334, 821, 1077, 11, 34, 12, 10, 12], [], ['scale'],
          [('distance', (0, 1)), ('dihedral', (0, 1, 2, 3)), ('angle', (2, 3, 4)), ('z', (4,)), ('z', (0,))]),
 'harmonic-angle': ([0, 310, 12, 53, 54, 11, 528, 12], ['0x1.0000000000000p-1'], [], [('angle', (0, 1, 2))]),
 'harmonic-bond': ([0, 310, 12, 53, 54, 11, 528, 12], ['0x1.0000000000000p-1'], [], [('distance', (0, 1))]),
 'periodic-torsion': ([566, 0, 54, 53, 12, 310, 11, 24, 10, 12], ['0x1.0000000000000p+0'], [], [('dihedral', (0, 1, 2, 3))]),
 'sixteen': ([54, 53, 310, 11, 528, 309, 310, 11, 528, 10, 565, 310, 11, 528, 10, 821, 310, 11, 528, 10, 1077, 310, 11, 528, 10, 0, 1333, 310, 11,
              528, 12, 10, 12, 566, 1589, 822, 11, 528, 1845, 822, 11, 528, 10, 2101, 822, 11, 528, 10, 2357, 822, 11, 528, 10, 12, 10, 1078, 2613,
              1334, 11, 24, 256, 2869, 12, 24, 10, 12, 10, 1590, 3125, 3381, 11, 1846, 11, 528, 3637, 1, 11, 528, 10, 3893, 257, 11, 528, 10, 12,
              10],
             ['0x1.47ae147ae147bp-7', '0x1.0000000000000p+1'], ['y0', 'z0'],
             [('distance', (0, 1)), ('distance', (1, 2)), ('distance', (2, 3)), ('distance', (4, 5)), ('distance', (6, 7)), ('distance', (0, 7)),
              ('angle', (0, 1, 2)), ('angle', (1, 2, 3)), ('angle', (4, 5, 6)), ('angle', (5, 6, 7)), ('dihedral', (0, 1, 2, 3)),
              ('dihedral', (4, 5, 6, 7)), ('x', (7,)), ('x', (0,)), ('y', (7,)), ('z', (7,))]),
 'stretch-bend': ([1, 54, 12, 7, 6, 53, 310, 11, 12, 309, 566, 11, 565, 822, 11, 10, 12], [], ['scale'],
                  [('angle', (0, 1, 2)), ('distance', (0, 1)), ('distance', (2, 1))]),
 'torsion-14': ([566, 0, 54, 53, 12, 310, 11, 24, 10, 12, 256, 1078, 12, 309, 822, 11, 528, 12, 10], ['0x1.0000000000000p+0', '0x1.0000000000000p-1'],
                [], [('dihedral', (0, 1, 2, 3)), ('distance', (0, 3))]),
 'urey-bradley': ([0, 310, 12, 53, 54, 11, 528, 12, 0, 822, 12, 309, 566, 11, 528, 12, 10], ['0x1.0000000000000p-1'], [],
                  [('angle', (0, 1, 2)), ('distance', (0, 2))])}
