"""GPU tests of the tabulated functions of a CustomNonbondedForce on the pair-expression kernel (csrc/pair_expr.hip; the words TAB_C1,
TAB_D1, TAB_D2 of csrc/pair_expr_vm.h): Continuous1DFunction, Discrete1DFunction and Discrete2DFunction called from an energy text.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 max|F|.  References (tests/pair_table_cases.py):
scipy's natural cubic spline -- the specification of a Continuous1DFunction -- and a fp64 O(N^2) minimum-image sum over closed-form
radial functions in numpy; the same context running the mixing-rule text where there is one.

Worst deviations measured on an MI355X: MEASURED_DEVIATIONS below."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import pair_expr_cases as P  # noqa: E402
import pair_table_cases as C  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd import tables as T  # noqa: E402

E_REL, F_REL = 1e-10, 1e-9
MEASURED_DEVIATIONS = """
one pair on a 6-knot spline (between knots, at a knot, r = min, r = max; 1 .. 64 lanes): energy rel <= 6.0e-16, force rel <= 1.7e-15
three atoms, g(type1,type2)*exp(-r) + f(type1)*f(type2)/r: energy rel 1.3e-16, forces 2.4e-16 of max|F|
type-pair Buckingham tables against the mixing-rule text in the same context: the same bits (q-SPC-FW and HEAQ: energy and forces)
type-pair Buckingham tables against the closed-form sum: energy rel < 1e-16 (both); forces 2.1e-15 (q-SPC-FW), 4.4e-15 (HEAQ) of max|F|
... with an off-diagonal entry no mixing rule gives: energy rel < 1e-16, 1.5e-16; forces 2.1e-15, 4.8e-15 of max|F|
eps1*eps2*U(r), 901 knots, against the sum over the scipy spline: energy rel 2.0e-16, forces 1.3e-14 of max|F| (switched: < 1e-16, 1.3e-14)
U tabulated from 0.2 nm: energy rel < 1e-16 (both); forces 2.1e-14 (q-SPC-FW), 2.4e-14 (HEAQ) of max|F|
20 Verlet steps of 0.1 fs from rest (an unrelaxed box: potential energy pours into motion, atoms move up to 0.055 nm):
|E(20) - E(0)| = 4.303e3 kJ/mol of E(0) = 3.455e5 with the tables and 4.303e3 kJ/mol with the mixing-rule text
"""


def assert_close(e, f, e_ref, f_ref, what, e_rel=E_REL):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= e_rel * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos, energy=True, fill=0.0):
    f = dev(np.full((len(pos), 3), fill))
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


BOX = np.full(3, 4.0)


# ------------------------------------------------------------------------------------ through the API
def table_system(data, text, names, params, functions, rc, rswitch=None, extra=None):
    """A System whose force 0 (group 0) is CustomNonbondedForce(text) with `functions` [(name, function)], CutoffPeriodic, the fixture's
    exclusions.  extra: (text, names, params) of a second force in group 1 over the same particles and exclusions."""
    n = len(data['positions'])
    system = openmm.System()
    for m in data['mass']:
        system.addParticle(float(m))
    L = data['box']
    system.setDefaultPeriodicBoxVectors((float(L[0]), 0, 0), (0, float(L[1]), 0), (0, 0, float(L[2])))
    made = []
    for group, (txt, nms, prm, fns) in enumerate([(text, names, params, functions)] + ([extra + ([],)] if extra else [])):
        force = openmm.CustomNonbondedForce(txt)
        for name in nms:
            force.addPerParticleParameter(name)
        for name, fn in fns:
            force.addTabulatedFunction(name, fn)
        for row in np.asarray(prm, dtype=np.float64).reshape(n, len(nms)):
            force.addParticle([float(v) for v in row])
        for i, j in data['exc_pairs']:
            force.addExclusion(int(i), int(j))
        force.setNonbondedMethod(force.CutoffPeriodic)
        force.setCutoffDistance(rc)
        if rswitch is not None:
            force.setUseSwitchingFunction(True)
            force.setSwitchingDistance(rswitch)
        force.setForceGroup(group)
        system.addForce(force)
        made.append(force)
    return system, made


def context_with(system, data, dt=0.001):
    context = openmm.Context(system, openmm.VerletIntegrator(dt))
    context.setPositions(data['positions'] * unit.nanometers)
    return context


def energy_forces(context, group=0):
    state = context.getState(getEnergy=True, getForces=True, groups={group})
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def entry_of(context, force):
    (entry,) = [e for e in context._engine.entries if e.force is force]
    return entry


# ------------------------------------------------------------------------------------ 1. fails without the feature
KNOTS6 = [9.0, 4.0, 2.5, 1.0, 0.75, 0.5]          # on [0.2, 0.45]: knots every 0.05 nm


def one_pair(r, values=KNOTS6, lo=0.2, hi=0.45, lanes=None, rc=0.9):
    """(E, forces) of two atoms r apart along x under U(r), through the API (on the parent commit: AttributeError at
    addTabulatedFunction).  Atom 0 sits at x = 0, so the difference of the coordinates IS the double r -- and sqrt(r * r) gives it
    back -- where r = min, r = max and a knot are meant exactly."""
    system = openmm.System()
    for _ in range(2):
        system.addParticle(12.0)
    system.setDefaultPeriodicBoxVectors((4.0, 0, 0), (0, 4.0, 0), (0, 0, 4.0))
    force = openmm.CustomNonbondedForce('U(r)')
    force.addTabulatedFunction('U', openmm.Continuous1DFunction(values, lo, hi))
    force.addParticle([])
    force.addParticle([])
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(rc)
    system.addForce(force)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    if lanes is not None:
        context._engine.ctx.set_option('lanes_per_row', lanes)
    context.setPositions(np.array([[0.0, 1.0, 2.0], [r, 1.0, 2.0]]) * unit.nanometers)
    e, f = energy_forces(context)
    if lanes is not None:
        assert context._engine.ctx.pair_stats(entry_of(context, force).pair_ids[0])['lanes_per_atom'] == lanes
    context._engine.ctx.check()
    return e, f


@pytest.mark.parametrize('lanes', [None, 1, 2, 4, 8, 16, 64])
def test_one_pair_on_a_spline(lanes):
    s, d = C.reference_spline(KNOTS6, 0.2, 0.45)
    inside = {'between knots': 0.31, 'at a knot': 0.2 + 2 * (0.45 - 0.2) / 5, 'r = min': 0.2, 'r = max': 0.45}
    if lanes is not None:
        inside = {'between knots': 0.31}
    for what, r0 in inside.items():
        e, f = one_pair(r0, lanes=lanes)
        e_ref, de_ref = float(s(r0)), float(d(r0))
        print('%s (lanes %s): r = %.17g  E = %.16g (spline %.16g, rel %.1e)  F = %.16g (-S\' = %.16g, rel %.1e)' %
              (what, lanes, r0, e, e_ref, abs(e - e_ref) / abs(e_ref), f[1, 0], -de_ref, abs(f[1, 0] + de_ref) / abs(de_ref)))
        assert math.isfinite(e) and abs(e - e_ref) <= E_REL * abs(e_ref)
        assert abs(f[1, 0] + de_ref) <= F_REL * abs(de_ref) and f[0, 0] == -f[1, 0] and not f[:, 1:].any()
    if lanes is None:
        for r0 in (0.199, 0.451):          # outside the table: zeros, not small numbers
            e, f = one_pair(r0)
            assert e == 0.0 and not f.any()


def test_two_knots_are_a_straight_line():
    e, f = one_pair(0.3, values=[3.0, 1.0], lo=0.2, hi=0.6)
    r = 0.3
    assert e == pytest.approx(3.0 - 5.0 * (r - 0.2), rel=E_REL) and f[1, 0] == pytest.approx(5.0, rel=F_REL) and f[0, 0] == -f[1, 0]


# ------------------------------------------------------------------------------------ 2. the discrete words at the smallest shape
def test_three_atoms_of_two_types_and_an_update():
    text = 'g(type1,type2)*exp(-r) + f(type1)*f(type2)/r'
    types = [0, 1, 1]
    gm = np.array([[1.5, -0.7], [-0.7, 2.25]])          # symmetric, three distinct values
    fv = np.array([0.5, 1.25])
    pos = np.array([[1.0, 1.0, 1.0], [1.3, 1.0, 1.0], [1.0, 1.4, 1.1]])
    system = openmm.System()
    for _ in types:
        system.addParticle(12.0)
    system.setDefaultPeriodicBoxVectors((4.0, 0, 0), (0, 4.0, 0), (0, 0, 4.0))
    force = openmm.CustomNonbondedForce(text)
    force.addPerParticleParameter('type')
    g = openmm.Discrete2DFunction(2, 2, gm.T.reshape(-1))          # values[i + xsize*j]
    force.addTabulatedFunction('g', g)
    force.addTabulatedFunction('f', openmm.Discrete1DFunction(fv))
    for t in types:
        force.addParticle([t])
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(0.9)
    system.addForce(force)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(pos * unit.nanometers)

    def closed_form(gm):
        e_ref, f_ref = 0.0, np.zeros((3, 3))
        for i in range(3):
            for j in range(i + 1, 3):
                d = pos[i] - pos[j]
                r = float(np.sqrt(d @ d))
                gg, ff = gm[types[i], types[j]], fv[types[i]] * fv[types[j]]
                e_ref += gg * math.exp(-r) + ff / r
                de = -gg * math.exp(-r) - ff / (r * r)
                f_ref[i] -= de * d / r
                f_ref[j] += de * d / r
        return e_ref, f_ref

    e, f = energy_forces(context)
    assert_close(e, f, *closed_form(gm), 'three atoms')
    pid = entry_of(context, force).pair_ids[0]
    builds = context._engine.ctx.pair_stats(pid)['n_builds']
    changed = gm.copy()
    changed[0, 1] = changed[1, 0] = 4.5
    g.setFunctionParameters(2, 2, changed.T.reshape(-1))
    force.updateParametersInContext(context)
    e2, f2 = energy_forces(context)
    assert abs(e2 - e) > 1.0
    assert_close(e2, f2, *closed_form(changed), 'three atoms, g(0,1) = 4.5')
    assert context._engine.ctx.pair_stats(pid)['n_builds'] == builds          # new numbers, the same list
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 3. type-pair Buckingham
TABLE_TEXT = 'A(t1,t2)*exp(-B(t1,t2)*r) - C(t1,t2)/r^6'
PAIRS = dict(spcfw=314034, heaq=171421)
ATOMS = dict(spcfw=(1536, 2), heaq=(1083, 4))


def matrix_functions(A, Bm, Cm):
    n = len(A)
    return [(name, openmm.Discrete2DFunction(n, n, m.T.reshape(-1))) for name, m in (('A', A), ('B', Bm), ('C', Cm))]


@pytest.mark.parametrize('fixture', ['spcfw', 'heaq'])
def test_type_pair_buckingham(request, fixture):
    data = request.getfixturevalue(fixture)
    rc = P.CUTOFF[fixture]
    case = P.TEXTS['buckingham']
    kind, rows, A, Bm, Cm = C.buckingham_tables(data['mass'])
    assert (len(kind), len(A)) == ATOMS[fixture]
    system, (tabled, mixing) = table_system(data, TABLE_TEXT, ['t'], kind, matrix_functions(A, Bm, Cm), rc,
                                            extra=(case['text'], case['names'], rows))
    context = context_with(system, data)
    engine = context._engine
    e, f = energy_forces(context, 0)
    e_mix, f_mix = energy_forces(context, 1)
    entry = entry_of(context, tabled)
    assert X.table_words(entry.program.code) == [('TAB_D2', 0), ('TAB_D2', 1), ('TAB_D2', 2)]
    # the input checks itself
    assert engine.ctx.pair_count_within(entry.pair_ids[0], engine.x, rc) // 2 == PAIRS[fixture]
    assert_close(e, f, e_mix, f_mix, '%s / tables against the mixing-rule text' % fixture)
    e_ref, f_ref, counted = C.radial_sum(C.buckingham_radial(kind, A, Bm, Cm), data['positions'], data['box'], rc, data['exc_pairs'])
    assert counted == PAIRS[fixture]
    assert_close(e, f, e_ref, f_ref, '%s / tables against the closed-form sum' % fixture)
    # one off-diagonal entry of each table becomes a value no mixing rule gives (an NBFIX): against the closed form only
    a, b = 0, len(A) - 1
    for m, factor in ((A, 1.37), (Bm, 0.91), (Cm, 2.3)):
        m[a, b] = m[b, a] = factor * m[a, b]
    for k, m in enumerate((A, Bm, Cm)):
        tabled.getTabulatedFunction(k).setFunctionParameters(len(A), len(A), m.T.reshape(-1))
    tabled.updateParametersInContext(context)
    e2, f2 = energy_forces(context, 0)
    e_ref, f_ref, _ = C.radial_sum(C.buckingham_radial(kind, A, Bm, Cm), data['positions'], data['box'], rc, data['exc_pairs'])
    assert abs(e2 - e) > 1e-3 * abs(e)
    assert_close(e2, f2, e_ref, f_ref, '%s / tables with an off-diagonal override' % fixture)
    engine.ctx.check()


# ------------------------------------------------------------------------------------ 4. a tabulated radial potential at size
def eps_by_type(mass):
    kind, ntypes = C.types_by_mass(mass)
    return np.random.default_rng(P.SEED).uniform(0.5, 1.5, ntypes)[kind]


def spline_radial(eps, s, d):
    return lambda i, j, r: (eps[i] * eps[j] * s(r), eps[i] * eps[j] * d(r))


def test_tabulated_potential_at_size(spcfw):
    lo, hi, rc = 0.14, 1.0, P.CUTOFF['spcfw']
    values = C.tabulated_u(lo, hi)
    s, d = C.reference_spline(values, lo, hi)
    eps = eps_by_type(spcfw['mass'])
    _, _, r_all, _ = P.pairs_within(spcfw['positions'], spcfw['box'], rc, spcfw['exc_pairs'])
    assert len(r_all) == PAIRS['spcfw'] and lo < r_all.min() and abs(r_all.min() - 0.1469) < 5e-5          # every pair is in range
    for rswitch in (None, 0.9):
        system, (force,) = table_system(spcfw, 'eps1*eps2*U(r)', ['eps'], eps, [('U', openmm.Continuous1DFunction(values, lo, hi))], rc, rswitch)
        context = context_with(system, spcfw)
        e, f = energy_forces(context)
        e_ref, f_ref, counted = C.radial_sum(spline_radial(eps, s, d), spcfw['positions'], spcfw['box'], rc, spcfw['exc_pairs'], rswitch)
        assert counted == PAIRS['spcfw']
        assert_close(e, f, e_ref, f_ref, 'q-SPC-FW / eps1*eps2*U(r), 901 knots' + (', switch 0.9 -> 1.0' if rswitch else ''))
        assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()
        context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 5. out of range is zero, not garbage
@pytest.mark.parametrize('fixture,below', [('spcfw', 885), ('heaq', 621)])
def test_pairs_below_the_table_contribute_nothing(request, fixture, below):
    data = request.getfixturevalue(fixture)
    lo, hi, rc = 0.2, 1.0, P.CUTOFF[fixture]
    values = C.tabulated_u(lo, hi)
    s, d = C.reference_spline(values, lo, hi)
    eps = eps_by_type(data['mass'])
    _, _, r_all, _ = P.pairs_within(data['positions'], data['box'], rc, data['exc_pairs'])
    assert int((r_all < lo).sum()) == below
    system, (force,) = table_system(data, 'eps1*eps2*U(r)', ['eps'], eps, [('U', openmm.Continuous1DFunction(values, lo, hi))], rc)
    context = context_with(system, data)
    e, f = energy_forces(context)
    e_ref, f_ref, counted = C.radial_sum(spline_radial(eps, s, d), data['positions'], data['box'], rc, data['exc_pairs'], r_from=lo)
    assert counted == PAIRS[fixture] - below
    assert_close(e, f, e_ref, f_ref, '%s / U tabulated from 0.2 nm, %d pairs below it' % (fixture, below))
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 6. same bits, and a short run
def test_same_bits_with_and_without_the_energy(spcfw):
    """All three words in one text: the forces of the evaluation with the energy and of the force-only one are the same bits, and so
    are two evaluations."""
    rc = P.CUTOFF['spcfw']
    kind, rows, A, Bm, Cm = C.buckingham_tables(spcfw['mass'])
    text = TABLE_TEXT + ' + 1e-3*w(t1)*w(t2)*U(r)'
    functions = matrix_functions(A, Bm, Cm) + [('w', openmm.Discrete1DFunction([0.8, 1.2])),
                                               ('U', openmm.Continuous1DFunction(C.tabulated_u(0.14, 1.0), 0.14, 1.0))]
    system, (force,) = table_system(spcfw, text, ['t'], kind, functions, rc)
    context = context_with(system, spcfw)
    engine = context._engine
    entry = entry_of(context, force)
    assert sorted(set(X.table_words(entry.program.code))) == [('TAB_C1', 4), ('TAB_D1', 3), ('TAB_D2', 0), ('TAB_D2', 1), ('TAB_D2', 2)]
    pid = entry.pair_ids[0]

    def run(energy):
        f = torch.zeros((len(kind), 3), dtype=torch.float64, device='cuda')
        e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
        engine.ctx.force_eval(pid, engine.x, f, energy=e)
        engine.ctx.synchronize()
        return (e.item() if energy else None), f.cpu().numpy()
    e1, f1 = run(True)
    e2, f2 = run(True)
    _, f3 = run(False)
    assert e1 == e2 and np.array_equal(f1, f2), 'two evaluations differ'
    assert np.array_equal(f1, f3), 'the force-only evaluation gives other forces than the one with the energy'
    assert math.isfinite(e1) and np.isfinite(f1).all() and np.abs(f1).max() > 1.0
    engine.ctx.check()


def test_twenty_verlet_steps_conserve_energy_as_the_mixing_rule_text_does(spcfw):
    """20 steps of VerletIntegrator(0.1 fs) from rest under the type-pair Buckingham tables, and under the mixing-rule text that
    gives the same potential: the change of E = potential + kinetic energy is a measured value (MEASURED_DEVIATIONS) -- the two are
    asked to be of the same order of magnitude, no more."""
    rc = P.CUTOFF['spcfw']
    case = P.TEXTS['buckingham']
    kind, rows, A, Bm, Cm = C.buckingham_tables(spcfw['mass'])
    drifts = {}
    for which in ('tables', 'mixing'):
        if which == 'tables':
            system, _ = table_system(spcfw, TABLE_TEXT, ['t'], kind, matrix_functions(A, Bm, Cm), rc)
        else:
            system, _ = table_system(spcfw, case['text'], case['names'], rows, [], rc)
        context = context_with(system, spcfw, dt=0.0001)
        state = context.getState(getEnergy=True)
        e0 = state.getPotentialEnergy()._value + state.getKineticEnergy()._value
        context.getIntegrator().step(20)
        state = context.getState(getEnergy=True, getPositions=True)
        e20 = state.getPotentialEnergy()._value + state.getKineticEnergy()._value
        moved = np.abs(state.getPositions(asNumpy=True)._value - spcfw['positions']).max()
        drifts[which] = abs(e20 - e0)
        print('%s: E(0) = %.10g, E(20) = %.10g kJ/mol, |E(20) - E(0)| = %.3e, atoms moved up to %.2e nm' % (which, e0, e20, drifts[which], moved))
        assert math.isfinite(e20) and moved > 1e-5
        context._engine.ctx.check()
    assert 0.1 * drifts['mixing'] <= drifts['tables'] <= 10.0 * drifts['mixing']


# ------------------------------------------------------------------------------------ 7. refusals at the ABI
def test_library_refusals_launch_nothing():
    ctx = B.HipContext(2, BOX)
    try:
        pos = np.array([[1.0, 1.0, 1.0], [1.3, 1.0, 1.0]])
        u = (T.CONTINUOUS1D, 3, 1, 0.2, 0.8, T.spline_coefficients([4.0, 2.0, 1.0], 0.2, 0.8).reshape(-1))
        f1 = (T.DISCRETE1D, 2, 1, 0.0, 0.0, np.array([1.0, 2.0]))
        g2 = (T.DISCRETE2D, 2, 2, 0.0, 0.0, np.array([1.0, 2.0, 2.0, 3.0]))
        # a table word in a term program
        with pytest.raises(B.HipError, match='amm_term_expr_create: opcode 55 is not a term-expression op'):
            ctx.term_expr_create(0, [X.TERM_OPCODES['TERM_VAR'], X.TABLE_OPCODES['TAB_C1']], [], [], [[0, 1, -1, -1]], np.zeros((0, 1)))
        # ... and one whose index no force can have
        with pytest.raises(B.HipError, match='tabulated-function index out of range'):
            ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, 0.9), [X.PAIR_OPCODES['PAIR_R'], X.TABLE_OPCODES['TAB_C1'] | (8 << 8)], [], [], None, None, None)
        prog = X.compile_pair('g(t1,t2)*U(r)', ['t'], [], {'U': ('Continuous1D', 1), 'g': ('Discrete2D', 2)})
        fid = ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, 0.9), prog.code, prog.consts, [], np.array([0.0, 1.0]), None, None)
        # evaluation before the tables are set: a message, and the force buffer as it was
        sentinel = 12345.0
        with pytest.raises(B.HipError, match='reads tabulated functions and none are set'):
            evaluate(ctx, fid, pos, fill=sentinel)
        buf = dev(np.full((2, 3), sentinel))
        with pytest.raises(B.HipError, match='none are set'):
            ctx.force_eval(fid, dev(pos), buf)
        ctx.synchronize()
        assert (buf.cpu().numpy() == sentinel).all() and ctx.pair_stats(fid)['n_evals'] == 0
        # a missing table, another kind, another number of arguments
        with pytest.raises(B.HipError, match=r'word TAB_D2 \(57\) reads table 1: 1 given'):
            ctx.pair_expr_set_tables(fid, [u])
        with pytest.raises(B.HipError, match=r'word TAB_C1 \(55\) takes a Continuous1DFunction \(1 argument\), table 0 is a Discrete1DFunction'):
            ctx.pair_expr_set_tables(fid, [f1, g2])
        with pytest.raises(B.HipError, match=r'word TAB_D2 \(57\) takes a Discrete2DFunction \(2 arguments\), table 1 is a Discrete1DFunction'):
            ctx.pair_expr_set_tables(fid, [u, f1])
        with pytest.raises(B.HipError, match='none are set'):          # (nothing was kept from the refused calls)
            ctx.force_eval(fid, dev(pos), buf)
        ctx.pair_expr_set_tables(fid, [u, g2])
        e, f = evaluate(ctx, fid, pos)
        s, d = C.reference_spline([4.0, 2.0, 1.0], 0.2, 0.8)
        r = float(pos[1, 0] - pos[0, 0])
        assert e == pytest.approx(2.0 * float(s(r)), rel=E_REL) and f[1, 0] == pytest.approx(-2.0 * float(d(r)), rel=F_REL)
        # a re-upload carries values, not sizes
        with pytest.raises(B.HipError, match='table 0 changed its kind or size'):
            ctx.pair_expr_set_tables(fid, [(T.CONTINUOUS1D, 4, 1, 0.2, 0.8, T.spline_coefficients([4.0, 2.0, 1.0, 0.5], 0.2, 0.8).reshape(-1)), g2])
        with pytest.raises(B.HipError, match='their number cannot change'):
            ctx.pair_expr_set_tables(fid, [u, g2, f1])
        e2, f2 = evaluate(ctx, fid, pos)
        assert e2 == e and np.array_equal(f2, f)          # the refused uploads changed nothing
        ctx.pair_expr_set_tables(fid, [u, (T.DISCRETE2D, 2, 2, 0.0, 0.0, np.array([1.0, 5.0, 5.0, 3.0]))])
        e3, _ = evaluate(ctx, fid, pos)
        assert e3 == pytest.approx(2.5 * e, rel=1e-15)
        # an index outside its table is NaN for that pair, never a read outside the table
        ctx.pair_set_params(fid, np.array([0.0, 7.0]), np.zeros(2), np.zeros(2))
        e4, f4 = evaluate(ctx, fid, pos)
        assert math.isnan(e4) and np.isnan(f4[:, 0]).all()
        # a force of another family takes no tables
        q = np.array([1.0, 2.0])
        other = ctx.pair_create(B.pair_desc(B.NEAR_NONE, 1.0, rc0=1.0, rs0=0.8), q, q, q)
        with pytest.raises(B.HipError, match='not a pair-expression force'):
            ctx.pair_expr_set_tables(other, [u])
    finally:
        ctx.close()
