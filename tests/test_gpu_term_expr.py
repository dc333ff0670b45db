"""GPU tests of the term-expression forces (csrc/term_expr.hip): a CustomBondForce / CustomAngleForce / CustomTorsionForce /
CustomExternalForce whose energy text is none of the hand-written kinds, compiled on the host and interpreted per term.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 max|F|.  References: the CPU oracle and the
hand-written GPU kinds for texts that restate one, tests/term_expr_cases.py (the text at 50 digits, forces by mpmath.diff in every
Cartesian coordinate) for texts no kind covers, closed forms for the smallest shapes.  Dynamics: 1e-12 nm against the hand-written
kinds over the horizons given.

Worst deviations measured on an MI355X: restated kinds on emim-BCN4 against the oracle -- energy rel 7.9e-16, forces
9.4e-15 of max|F|; against the hand-written GPU kinds -- 2.3e-16 and 1.9e-13 (the angles; bonds 8.6e-15, torsions 1.2e-16); texts
no kind covers against the 50-digit reference -- energy rel 4.0e-15 (Morse), forces 6.5e-15 of max|F| (Morse); 20 Verlet steps
of q-SPC-FW with custom bond and angle texts against the harmonic kinds: 1.2e-14 nm;
10 RESPA [4, 2, 1] steps of emim-BCN4 with a custom torsion text against PeriodicTorsionForce: 2.2e-16 nm; 4 RESPA steps of
q-SPC-FW on the plain path against the fused inner loop: 4.4e-16 nm."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import term_expr_cases as T  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

E_REL, F_REL = 1e-10, 1e-9


def assert_close(e, f, e_ref, f_ref, what, e_rel=E_REL):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= e_rel * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


# ------------------------------------------------------------------------------------ through the API
CLASSES = {T.BOND: ('CustomBondForce', 'addPerBondParameter', 'addBond'), T.ANGLE: ('CustomAngleForce', 'addPerAngleParameter', 'addAngle'),
           T.TORSION: ('CustomTorsionForce', 'addPerTorsionParameter', 'addTorsion'),
           T.EXTERNAL: ('CustomExternalForce', 'addPerParticleParameter', 'addParticle')}


def custom_force(name, idx, params, periodic=False, group=0, gvalues=None):
    """The OpenMM-shaped force of text `name` over the index rows `idx` with parameter rows `params`."""
    case = T.TEXTS[name]
    cls, add_name, add_term = CLASSES[case['kind']]
    force = getattr(openmm, cls)(case['text'])
    for p in case['names']:
        getattr(force, add_name)(p)
    for g, value in (case['globals'] if gvalues is None else gvalues).items():
        force.addGlobalParameter(g, value)
    for atoms, row in zip(idx, params):
        getattr(force, add_term)(*[int(a) for a in atoms], [float(v) for v in row])
    if case['kind'] != T.EXTERNAL:
        force.setUsesPeriodicBoundaryConditions(periodic)
    force.setForceGroup(group)
    return force


def bare_system(masses, box=None):
    system = openmm.System()
    for m in masses:
        system.addParticle(float(m))
    if box is not None:
        system.setDefaultPeriodicBoxVectors((float(box[0]), 0, 0), (0, float(box[1]), 0), (0, 0, float(box[2])))
    return system


def context_with(system, positions, integrator=None):
    context = openmm.Context(system, integrator or openmm.VerletIntegrator(0.001))
    context.setPositions(np.asarray(positions) * unit.nanometers)
    return context


def energy_forces(context, **kw):
    state = context.getState(getEnergy=True, getForces=True, **kw)
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def positions_of(context):
    return context.getState(getPositions=True).getPositions(asNumpy=True)._value


def harmonic_rows(data):
    """(index rows, parameter rows) of the three restated kinds over a fixture's bonds, angles and torsions."""
    return {'harmonic-bond': (data['bonds'], np.stack([data['bond_r0'], data['bond_k']], axis=1)),
            'harmonic-angle': (data['angles'], np.stack([data['angle_theta0'], data['angle_k']], axis=1)),
            'periodic-torsion': (data['torsions'], np.stack([data['torsion_n'].astype(float), data['torsion_phase'], data['torsion_k']], axis=1))}


# ------------------------------------------------------------------------------------ 1. fails without the feature
def test_morse_bonds_custom_torsions_and_external_forces_run_in_a_context(spcfw, emim):
    """On the parent commit: InputError('energy expression not recognised by the HIP path ...') for the Morse bond, AttributeError
    for openmm.CustomTorsionForce and openmm.CustomExternalForce."""
    rng = np.random.default_rng(1)
    bonds = spcfw['bonds']
    morse = custom_force('morse', bonds, np.stack([rng.uniform(200, 500, len(bonds)), rng.uniform(15, 25, len(bonds)), spcfw['bond_r0']], axis=1),
                         periodic=True)
    system = bare_system(spcfw['mass'], spcfw['box'])
    system.addForce(morse)
    context = context_with(system, spcfw['positions'])
    e, f = energy_forces(context)
    (entry,) = context._engine.entries
    assert entry.term_expr and len(entry.term_ids) == 1 and entry.bonded_id is None and len(entry.program.code) == 12
    assert math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1.0
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()
    context._engine.ctx.check()
    torsions = emim['torsions']
    rb = custom_force('rb-torsion', torsions, rng.uniform(-10, 10, (len(torsions), 6)), periodic=True)
    pin = custom_force('position-restraint', np.arange(0, 2800, 7).reshape(-1, 1),
                       np.concatenate([np.full((400, 1), 1000.0), emim['positions'][::7] + 0.01], axis=1), group=1)
    system = bare_system(emim['mass'], emim['box'])
    system.addForce(rb)
    system.addForce(pin)
    context = context_with(system, emim['positions'])
    assert [e_.term_expr for e_ in context._engine.entries] == [True, True]
    e0, f0 = energy_forces(context, groups={0})
    e1, f1 = energy_forces(context, groups={1})
    assert math.isfinite(e0) and e0 != 0.0 and np.isfinite(f0).all() and np.abs(f0.sum(axis=0)).max() <= 1e-9 * np.abs(f0).max()
    # 400 restraints displaced by (0.01, 0.01, 0.01): the closed form, and a net force (an external force conserves no momentum)
    assert e1 == pytest.approx(400 * 0.5 * 1000.0 * 3e-4, rel=1e-9) and np.abs(f1[::7] - 10.0).max() < 1e-6 and not f1[1::7].any()
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 2. the hand-written kinds, restated
ORACLE = {'harmonic-bond': lambda i, p, x, L, per: O.harmonic_bonds(i, p[:, 0], p[:, 1], x, L, periodic=per),
          'harmonic-angle': lambda i, p, x, L, per: O.harmonic_angles(i, p[:, 0], p[:, 1], x, L, periodic=per),
          'periodic-torsion': lambda i, p, x, L, per: O.periodic_torsions(i, p[:, 0].astype(np.int32), p[:, 1], p[:, 2], x, L, periodic=per)}


def hand_written_force(name, idx, params, periodic):
    if name == 'harmonic-bond':
        force = openmm.HarmonicBondForce()
        for (i, j), (r0, k) in zip(idx, params):
            force.addBond(int(i), int(j), float(r0), float(k))
    elif name == 'harmonic-angle':
        force = openmm.HarmonicAngleForce()
        for (i, j, k_), (t0, k) in zip(idx, params):
            force.addAngle(int(i), int(j), int(k_), float(t0), float(k))
    else:
        force = openmm.PeriodicTorsionForce()
        for (a, b, c, d), (n, phase, k) in zip(idx, params):
            force.addTorsion(int(a), int(b), int(c), int(d), int(n), float(phase), float(k))
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('name', ['harmonic-bond', 'harmonic-angle', 'periodic-torsion'])
def test_restated_kinds_against_the_oracle_and_the_hand_written_kernels(emim, name, periodic):
    idx, params = harmonic_rows(emim)[name]
    assert len(idx) == {'harmonic-bond': 2700, 'harmonic-angle': 4300, 'periodic-torsion': 4100}[name]
    results = []
    for make in (lambda: custom_force(name, idx, params, periodic), lambda: hand_written_force(name, idx, params, periodic)):
        system = bare_system(emim['mass'], emim['box'])
        system.addForce(make())
        context = context_with(system, emim['positions'])
        results.append(energy_forces(context))
        context._engine.ctx.check()
        assert context._engine.entries[0].term_expr is (len(results) == 1)
    (e, f), (e_hand, f_hand) = results
    e_ref, f_ref = ORACLE[name](idx, params, emim['positions'], emim['box'], periodic)
    assert_close(e, f, e_ref, f_ref, 'emim / %s, periodic %s, against the oracle' % (name, periodic))
    assert_close(e, f, e_hand, f_hand, 'emim / %s, periodic %s, against the hand-written kind' % (name, periodic))


# ------------------------------------------------------------------------------------ 3. texts no kind covers
@pytest.fixture(scope='module')
def references():
    """(energy, forces) of tests/term_expr_cases.py per text, computed once and never written to."""
    made = {}

    def get(name, data, idx, params, box):
        if name not in made:
            e, f, _ = T.term_sum(T.TEXTS[name], idx, params, data['positions'], box)
            f.setflags(write=False)
            made[name] = (e, f)
        return made[name]
    return get


@pytest.mark.parametrize('name', T.GPU_CASES)
def test_texts_no_kind_covers(references, emim, name):
    case = T.TEXTS[name]
    idx, params = T.reference_terms(name, emim)
    assert len(idx) == T.GPU_TERMS and len(emim['positions']) == 2800
    periodic = case['kind'] != T.EXTERNAL
    system = bare_system(emim['mass'], emim['box'])
    system.addForce(custom_force(name, idx, params, periodic))
    context = context_with(system, emim['positions'])
    e, f = energy_forces(context)
    e_ref, f_ref = references(name, emim, idx, params, emim['box'] if periodic else None)
    assert_close(e, f, e_ref, f_ref, 'emim / %s (%d terms, %d code words)' % (name, len(idx), len(context._engine.entries[0].program.code)))
    if name == 'flat-bottom':
        anchored = int(idx[0][0])
        assert np.array_equal(params[0][2:5], emim['positions'][anchored])
        assert not f[anchored].any() and not np.isnan(f).any()          # exactly zero at the anchor, not NaN
        assert (np.abs(f[idx[:, 0]]).max(axis=1) > 0).sum() >= 8        # ... and some atoms outside their wells
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 4. the smallest shapes, at the C-ABI
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def abi_force(ctx, name, idx, params, periodic=False, gvalues=None):
    case = T.TEXTS[name]
    g = dict(case['globals'] if gvalues is None else gvalues)
    prog = X.compile_term(case['text'], T.VARIABLES[case['kind']], case['names'], g)
    rows = np.full((len(idx), 4), -1, dtype=np.int32)
    rows[:, :T.ARITY[case['kind']]] = np.asarray(idx).reshape(len(idx), -1)
    par = np.asarray(params, dtype=np.float64).reshape(len(idx), len(case['names'])).T
    return ctx.term_expr_create(case['kind'], prog.code, prog.consts, [g[k] for k in prog.globals_], rows, par, periodic=periodic)


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def morse(r, D, a, r0):
    """(E, dE/dr) in closed form."""
    x = np.exp(-a * (r - r0))
    return D * (1.0 - x) ** 2, 2.0 * D * a * x * (1.0 - x)


BOX = np.full(3, 4.0)


def test_one_term_in_a_two_atom_system():
    ctx = B.HipContext(2, BOX)
    try:
        fid = abi_force(ctx, 'morse', [[0, 1]], [[300.0, 20.0, 0.1]])
        pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.12, 1.0]])
        e, f = evaluate(ctx, fid, pos)
        e_ref, de = morse(0.12, 300.0, 20.0, 0.1)
        print('one Morse bond: E = %.15g (closed form %.15g), F = %.15g (closed form %.15g)' % (e, e_ref, f[1, 1], -de))
        assert e == pytest.approx(e_ref, rel=E_REL) and f[1, 1] == pytest.approx(-de, rel=F_REL) and f[0, 1] == -f[1, 1]
        assert not f[:, [0, 2]].any()
        # accumulate adds to what is there; the energy adds to the scalar
        e2, f2 = evaluate(ctx, fid, pos, accumulate=True, start=np.ones((2, 3)))
        assert np.array_equal(f2, f + 1.0)
        ctx.check()
    finally:
        ctx.close()


def test_257_terms_the_second_block_holds_one_lane():
    n = 258
    pos = np.stack([1.0 + 0.011 * np.arange(n), np.full(n, 2.0) + 0.003 * (np.arange(n) % 3), np.full(n, 2.0)], axis=1)
    idx = np.stack([np.arange(257), np.arange(1, 258)], axis=1)
    rng = np.random.default_rng(5)
    par = np.stack([rng.uniform(200, 500, 257), rng.uniform(15, 25, 257), rng.uniform(0.009, 0.013, 257)], axis=1)
    ctx = B.HipContext(n, BOX)
    try:
        e, f = evaluate(ctx, abi_force(ctx, 'morse', idx, par), pos)
        d = pos[idx[:, 0]] - pos[idx[:, 1]]
        r = np.sqrt((d * d).sum(axis=1))
        e_t, de = morse(r, par[:, 0], par[:, 1], par[:, 2])
        f_ref = np.zeros((n, 3))
        np.add.at(f_ref, idx[:, 0], (-de / r)[:, None] * d)
        np.add.at(f_ref, idx[:, 1], (de / r)[:, None] * d)
        assert_close(e, f, float(e_t.sum()), f_ref, '257 Morse bonds on a chain')
        assert f[257].any()              # the last atom belongs to the term of the second block alone
        ctx.check()
    finally:
        ctx.close()


def test_star_of_300_bonds_on_one_atom_twice_the_same_bits():
    rng = np.random.default_rng(6)
    u = rng.normal(size=(300, 3))
    pos = np.concatenate([[[2.0, 2.0, 2.0]], 2.0 + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0.09, 0.15, (300, 1))])
    idx = np.stack([np.zeros(300, dtype=int), np.arange(1, 301)], axis=1)
    par = np.stack([rng.uniform(200, 500, 300), rng.uniform(15, 25, 300), rng.uniform(0.09, 0.13, 300)], axis=1)
    ctx = B.HipContext(301, BOX)
    try:
        fid = abi_force(ctx, 'morse', idx, par)
        e, f = evaluate(ctx, fid, pos)
        again = evaluate(ctx, fid, pos)
        _, f_only = evaluate(ctx, fid, pos, energy=False)
        assert again[0] == e and np.array_equal(again[1], f) and np.array_equal(f_only, f)
        d = pos[0] - pos[1:]
        r = np.sqrt((d * d).sum(axis=1))
        e_t, de = morse(r, par[:, 0], par[:, 1], par[:, 2])
        f_ref = np.concatenate([[((-de / r)[:, None] * d).sum(axis=0)], (de / r)[:, None] * d])
        scale = np.abs(f_ref).max()
        print('star of 300: E rel %.2e, central atom |dF| = %.2e of max|F|' % (abs(e - e_t.sum()) / e_t.sum(), np.abs(f[0] - f_ref[0]).max() / scale))
        assert abs(e - e_t.sum()) <= E_REL * e_t.sum() and np.abs(f - f_ref).max() <= F_REL * scale
        ctx.check()
    finally:
        ctx.close()


def test_three_restrained_atoms_of_a_thousand_every_other_row_is_zero():
    n = 1000
    rng = np.random.default_rng(7)
    pos = rng.uniform(0.0, 4.0, (n, 3))
    ctx = B.HipContext(n, BOX)
    try:
        everyone = abi_force(ctx, 'position-restraint', np.arange(n).reshape(-1, 1), np.concatenate([np.full((n, 1), 500.0), pos + 0.1], axis=1))
        who = np.array([3, 500, 999])
        anchors = pos[who] - 0.02
        three = abi_force(ctx, 'position-restraint', who.reshape(-1, 1), np.concatenate([np.full((3, 1), 1000.0), anchors], axis=1))
        _, stale = evaluate(ctx, everyone, pos + 0.05)
        assert np.abs(stale).min() > 1.0                        # every row of the buffer holds a value of another configuration
        e, f = evaluate(ctx, three, pos, start=stale)           # accumulate = 0: the force writes all rows
        others = np.setdiff1d(np.arange(n), who)
        assert not f[others].any()
        assert np.abs(f[who] + 1000.0 * 0.02).max() <= F_REL * 20.0 and e == pytest.approx(3 * 0.5 * 1000.0 * 3 * 0.02 ** 2, rel=E_REL)
        ctx.check()
    finally:
        ctx.close()


def test_zero_and_eight_per_term_parameters():
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.2], [1.3, 1.0, 1.2]])
    ctx = B.HipContext(3, BOX)
    try:
        prog = X.compile_term('g*(r-0.25)^2', ('r',), [], ['g'])
        rows = np.array([[0, 1, -1, -1], [1, 2, -1, -1]], dtype=np.int32)
        fid = ctx.term_expr_create(B.TERM_BOND, prog.code, prog.consts, [100.0], rows, np.zeros((0, 2)))
        e, f = evaluate(ctx, fid, pos)
        assert e == pytest.approx(100.0 * (0.05 ** 2 + 0.05 ** 2), rel=1e-12) and f[0, 2] == pytest.approx(-10.0, rel=1e-12)
        names = ['p%d' % k for k in range(8)]
        text = 'p0*r + p1*r^2 + p2*r^3 + p3 + p4*r^4 + p5/r + p6*sqrt(r) + p7*exp(-r)'
        prog = X.compile_term(text, ('r',), names, [])
        par = np.arange(1.0, 17.0).reshape(2, 8)          # term-major rows -> parameter-major for the call
        fid = ctx.term_expr_create(B.TERM_BOND, prog.code, prog.consts, [], rows, par.T)
        e, f = evaluate(ctx, fid, pos)

        def closed(r, p):
            return (p[0] * r + p[1] * r ** 2 + p[2] * r ** 3 + p[3] + p[4] * r ** 4 + p[5] / r + p[6] * math.sqrt(r) + p[7] * math.exp(-r),
                    p[0] + 2 * p[1] * r + 3 * p[2] * r ** 2 + 4 * p[4] * r ** 3 - p[5] / r ** 2 + 0.5 * p[6] / math.sqrt(r) - p[7] * math.exp(-r))
        (e0, d0), (e1, d1) = closed(0.2, par[0]), closed(0.3, par[1])
        print('eight parameters: E = %.15g (closed form %.15g)' % (e, e0 + e1))
        assert e == pytest.approx(e0 + e1, rel=E_REL) and f[0, 2] == pytest.approx(d0, rel=F_REL) and f[2, 0] == pytest.approx(-d1, rel=F_REL)
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 5. the periodic flag
def test_terms_across_a_box_face():
    """A bond, an angle and a torsion whose atoms straddle the face x = 0 of a 4 nm box: with the flag, the numbers of the unwrapped
    copy; without it, those of the raw coordinates."""
    whole = np.array([[0.05, 1.0, 1.0], [-0.06, 1.08, 1.0], [-0.10, 1.20, 1.07], [0.02, 1.28, 1.15]])
    wrapped = whole.copy()
    wrapped[whole[:, 0] < 0, 0] += 4.0
    cases = [('harmonic-bond', [[0, 1]], [[0.1, 3e5]]), ('cosine-angle', [[0, 1, 2]], [[1.9, 400.0]]),
             ('rb-torsion', [[0, 1, 2, 3]], [[1.0, -2.0, 3.0, -4.0, 5.0, -6.0]])]
    ctx = B.HipContext(4, BOX)
    try:
        for name, idx, par in cases:
            on, off = abi_force(ctx, name, idx, par, periodic=True), abi_force(ctx, name, idx, par, periodic=False)
            e_whole, f_whole = evaluate(ctx, off, whole)
            e_on, f_on = evaluate(ctx, on, wrapped)
            e_ref, f_ref, _ = T.term_sum(T.TEXTS[name], idx, par, whole)
            assert_close(e_whole, f_whole, e_ref, f_ref, name + ', unwrapped copy')
            assert_close(e_on, f_on, e_ref, f_ref, name + ', across the face with the flag')
            e_off, f_off = evaluate(ctx, off, wrapped)
            e_raw, f_raw, _ = T.term_sum(T.TEXTS[name], idx, par, wrapped)
            assert_close(e_off, f_off, e_raw, f_raw, name + ', across the face without the flag (raw distances)')
            assert abs(e_off - e_on) > 1e-3 * abs(e_on)
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 6. in one group with other forces
def test_one_group_with_a_nonbonded_and_a_bond_force(emim):
    idx, params = harmonic_rows(emim)['periodic-torsion']

    def build(groups):
        system = system_from_arrays(emim, nonbondedMethod='CutoffPeriodic')
        keep = [f for f in system.getForces() if isinstance(f, (openmm.NonbondedForce, openmm.HarmonicBondForce))]
        system._forces[:] = keep + [custom_force('periodic-torsion', idx, params, periodic=True)]
        for force, g in zip(system.getForces(), groups):
            force.setForceGroup(g)
        return context_with(system, emim['positions'])
    together, apart = build((0, 0, 0)), build((1, 2, 3))
    assert [type(e.force).__name__ for e in together._engine.entries] == ['HarmonicBondForce', 'NonbondedForce', 'CustomTorsionForce']
    e_all, f_all = energy_forces(together, groups={0})
    parts = [energy_forces(apart, groups={g}) for g in (1, 2, 3)]
    f_sum = parts[0][1] + parts[1][1] + parts[2][1]
    e_sum = sum(p[0] for p in parts)
    assert_close(e_all, f_all, e_sum, f_sum, 'one group against three')
    assert all(p[0] != 0.0 for p in parts) and energy_forces(apart)[0] == pytest.approx(e_sum, rel=1e-12)
    # the group as the scheduler evaluates it (EVAL of group 0, first member writes, the term-expression force adds last)
    engine = together._engine
    index, slot, _ = engine._define_group(0)
    engine.ctx.run_ops([B.Op(B.OP_EVAL, index, 0, 0, 0.0)])
    engine.ctx.synchronize()
    f_group = engine._buffer('f0').cpu().numpy()
    print('EVAL of the group: max|dF| = %.2e of max|F|' % (np.abs(f_group - f_sum).max() / np.abs(f_sum).max()))
    assert np.abs(f_group - f_sum).max() <= F_REL * np.abs(f_sum).max()
    for context in (together, apart):
        context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 7. parameters
def test_globals_per_term_values_and_the_two_instantiations(spcfw):
    bonds = spcfw['bonds'][:300]
    rng = np.random.default_rng(8)
    par = np.stack([rng.uniform(200, 500, 300), spcfw['bond_r0'][:300]], axis=1)
    force = custom_force('morse-global', bonds, par, periodic=True)
    system = bare_system(spcfw['mass'], spcfw['box'])
    system.addForce(force)
    context = context_with(system, spcfw['positions'])
    d = spcfw['positions'][bonds[:, 0]] - spcfw['positions'][bonds[:, 1]]
    d -= spcfw['box'] * np.rint(d / spcfw['box'])
    r = np.sqrt((d * d).sum(axis=1))

    def closed(scale, a, D=par[:, 0], r0=par[:, 1]):
        return float((scale * morse(r, D, a, r0)[0]).sum())
    e, f = energy_forces(context)
    assert e == pytest.approx(closed(1.5, 12.0), rel=E_REL)
    context.setParameter('a', 18.0)
    context.setParameter('scale', 0.5)
    e2, f2 = energy_forces(context)
    print('globals: E(a = 12, scale = 1.5) = %.12g, E(a = 18, scale = 0.5) = %.12g (closed form %.12g)' % (e, e2, closed(0.5, 18.0)))
    assert e2 == pytest.approx(closed(0.5, 18.0), rel=E_REL) and e2 != e
    new = par.copy()
    new[::2, 0] *= 1.25
    new[1::2, 1] += 0.003
    for k, row in enumerate(new):
        force.setBondParameters(k, int(bonds[k, 0]), int(bonds[k, 1]), [float(v) for v in row])
    force.updateParametersInContext(context)
    e3, f3 = energy_forces(context)
    assert e3 == pytest.approx(closed(0.5, 18.0, new[:, 0], new[:, 1]), rel=E_REL) and e3 != e2
    # with and without the energy: the same bits
    f_only = context.getState(getForces=True).getForces(asNumpy=True)._value
    assert np.array_equal(f_only, f3) and np.abs(f3).max() > 1.0
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 8. dynamics through the scheduler's plain path
def with_custom_texts(system, data, kinds):
    """The System with its HarmonicBondForce / HarmonicAngleForce / PeriodicTorsionForce (those in `kinds`) written as custom texts."""
    rows = harmonic_rows(data)
    classes = {'harmonic-bond': openmm.HarmonicBondForce, 'harmonic-angle': openmm.HarmonicAngleForce,
               'periodic-torsion': openmm.PeriodicTorsionForce}
    for k, force in enumerate(list(system._forces)):
        for name in kinds:
            if type(force) is classes[name]:
                idx, params = rows[name]
                system._forces[k] = custom_force(name, idx, params, force.usesPeriodicBoundaryConditions(), force.getForceGroup())
    return system


def run_pair(make_system, make_integrator, data, steps, seed=2026):
    """Positions after `steps` steps of the System as it is and with custom texts, stepping both together; the largest difference."""
    kT = unit.MOLAR_GAS_CONSTANT_R._value * 300.0
    v0 = np.random.default_rng(seed).normal(size=data['positions'].shape) * np.sqrt(kT / data['mass'])[:, None]
    contexts, integrators = [], []
    for custom in (False, True):
        integrators.append(make_integrator())
        context = openmm.Context(make_system(custom), integrators[-1])
        context.setPositions(data['positions'] * unit.nanometers)
        context.setVelocities(v0)
        contexts.append(context)
    worst = 0.0
    for _ in range(steps):
        xs = []
        for context, integrator in zip(contexts, integrators):
            integrator.step(1)
            xs.append(positions_of(context))
        worst = max(worst, float(np.abs(xs[0] - xs[1]).max()))
    moved = float(np.abs(xs[0] - data['positions']).max())
    for context in contexts:
        context._engine.ctx.check()
    return worst, moved, contexts


def test_twenty_verlet_steps_with_custom_bond_and_angle_texts(spcfw):
    def make(custom):
        system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
        return with_custom_texts(system, spcfw, ('harmonic-bond', 'harmonic-angle')) if custom else system
    worst, moved, contexts = run_pair(make, lambda: openmm.VerletIntegrator(0.001), spcfw, 20)
    assert [sum(e.term_expr for e in c._engine.entries) for c in contexts] == [0, 2]
    print('20 Verlet steps, custom bond and angle texts against the harmonic kinds: max |dx| = %.3e nm, atoms moved up to %.3e nm' % (worst, moved))
    assert moved > 1e-3 and worst <= 1e-12


def test_ten_respa_steps_with_a_custom_torsion_in_group_zero(emim):
    def make(custom):
        system = system_from_arrays(emim, nonbondedMethod='CutoffPeriodic')
        if custom:
            with_custom_texts(system, emim, ('periodic-torsion',))
        return atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    worst, moved, contexts = run_pair(make, lambda: atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds), emim, 10)
    groups = [[(type(e.force).__name__, e.group) for e in c._engine.entries] for c in contexts]
    assert ('PeriodicTorsionForce', 0) in groups[0] and ('CustomTorsionForce', 0) in groups[1] and ('HarmonicBondForce', 0) in groups[1]
    print('10 RESPA [4, 2, 1] steps, custom torsion text against PeriodicTorsionForce: max |dx| = %.3e nm, atoms moved up to %.3e nm' % (worst, moved))
    assert moved > 1e-3 and worst <= 1e-12


def test_the_fused_inner_loop_declines_a_group_with_a_term_expression_force(spcfw):
    """Flexible water under RESPA [4, 2, 1]: with harmonic kinds the inner loop rides on the pair launches as their epilogue (the
    counter of amm_run_stats); with the same terms as custom texts every rule declines the group and it is evaluated member by member
    on the plain path -- the counter stays at 0 and the trajectory is the same."""
    def make(custom):
        system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
        if custom:
            with_custom_texts(system, spcfw, ('harmonic-bond', 'harmonic-angle'))
        return atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    worst, moved, contexts = run_pair(make, lambda: atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds), spcfw, 4)
    stats = [c._engine.ctx.run_stats() for c in contexts]
    print('run statistics, harmonic kinds: %s; custom texts: %s; max |dx| = %.3e nm' % (stats[0], stats[1], worst))
    assert stats[0]['epilogues'] > 0 and stats[1]['epilogues'] == 0
    assert stats[1]['scheduled'] > stats[0]['scheduled']
    assert moved > 1e-4 and worst <= 1e-12


# ------------------------------------------------------------------------------------ 9. around it
def restrained_phenol(phenol, barostat=False):
    """Phenol in water with its heavy atoms restrained (k = 1000 kJ/mol/nm^2) to where they are."""
    system = system_from_arrays(phenol, nonbondedMethod='CutoffPeriodic', cutoff=0.9)
    sizes = np.bincount(phenol['residue'])
    heavy = np.nonzero((sizes[phenol['residue']] > 3) & (phenol['mass'] > 1.5))[0]
    assert len(heavy) == 7
    system.addForce(custom_force('position-restraint', heavy.reshape(-1, 1),
                                 np.concatenate([np.full((len(heavy), 1), 1000.0), phenol['positions'][heavy]], axis=1)))
    if barostat:
        mc = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 1)
        mc.setRandomNumberSeed(11)
        system.addForce(mc)
    return system, heavy


def test_minimisation_with_position_restraints(phenol):
    system, heavy = restrained_phenol(phenol)
    sim = app.Simulation(app.Topology(len(phenol['positions'])), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    start = phenol['positions'] + np.random.default_rng(12).normal(scale=0.005, size=phenol['positions'].shape)
    sim.context.setPositions(start * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy(maxIterations=30)
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    x = positions_of(sim.context)
    print('minimisation with restraints: E %.6g -> %.6g kJ/mol, restrained atoms within %.3e nm of their anchors' %
          (e0, e1, np.abs(x[heavy] - phenol['positions'][heavy]).max()))
    assert math.isfinite(e1) and e1 < e0
    sim.context._engine.ctx.check()


def test_ten_barostat_attempts_with_position_restraints(phenol):
    system, _ = restrained_phenol(phenol, barostat=True)
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(system, phenol['positions'], integrator)
    context.setVelocitiesToTemperature(300.0, 5)
    integrator.step(10)
    stats = context._engine.barostat_stats
    print('barostat with restraints: %s' % (stats,))
    assert stats['attempts'] == 10 and np.isfinite(positions_of(context)).all()
    context._engine.ctx.check()


def test_free_space_system_with_a_custom_bond_force():
    pos = np.array([[0.0, 0.0, 0.0], [0.11, 0.0, 0.0], [0.11, 0.13, 0.0]])
    system = bare_system([12.0, 12.0, 12.0])
    nb = openmm.NonbondedForce()
    for _ in range(3):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.NoCutoff)
    system.addForce(nb)
    system.addForce(custom_force('morse', [[0, 1], [1, 2]], [[300.0, 20.0, 0.1], [250.0, 18.0, 0.12]]))
    context = context_with(system, pos)
    assert context._engine.free_space
    e, f = energy_forces(context)
    (e0, d0), (e1, d1) = morse(0.11, 300.0, 20.0, 0.1), morse(0.13, 250.0, 18.0, 0.12)
    assert e == pytest.approx(e0 + e1, rel=E_REL) and f[0, 0] == pytest.approx(d0, rel=F_REL) and f[2, 1] == pytest.approx(-d1, rel=F_REL)
    context._engine.ctx.check()


def test_refusals():
    # the engine's
    system = bare_system([12.0] * 4, BOX)
    force = openmm.CustomTorsionForce('k*theta^2')
    force.addGlobalParameter('k', 2.0)
    force.addTorsion(0, 1, 2, 3)
    system.addForce(force)
    context = context_with(system, [[1.0, 1.0, 1.0], [1.1, 1.0, 1.0], [1.1, 1.1, 1.0], [1.1, 1.1, 1.1]])
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, k\) of a CustomTorsionForce with a generic energy expression'):
        context._engine.energy_derivative('k')
    force.addEnergyParameterDerivative('k')
    with pytest.raises(NotImplementedError, match='addEnergyParameterDerivative'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    free = bare_system([12.0] * 3)
    nb = openmm.NonbondedForce()
    for _ in range(3):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.NoCutoff)
    free.addForce(nb)
    free.addForce(custom_force('morse', [[0, 1]], [[300.0, 20.0, 0.1]], periodic=True))
    with pytest.raises(atomsmm.InputError, match='periodic boundary'):
        openmm.Context(free, openmm.VerletIntegrator(0.001))
    # the library's
    ctx = B.HipContext(3, BOX)
    nobox = B.HipContext(3, None)
    try:
        fid = abi_force(ctx, 'morse', [[0, 1]], [[300.0, 20.0, 0.1]])
        for call in (lambda: ctx.bonded_add_terms(fid, B.BOND_HARMONIC, [[0, 1]], [[0.1, 1.0]]), lambda: ctx.bonded_finalize(fid),
                     lambda: ctx.bonded_release(fid)):
            with pytest.raises(B.HipError, match='term-expression force'):
                call()
        with pytest.raises(B.HipError, match='atom index 3 of term 0 is out of range'):
            abi_force(ctx, 'morse', [[0, 3]], [[300.0, 20.0, 0.1]])
        with pytest.raises(B.HipError, match='no periodic box'):
            abi_force(nobox, 'morse', [[0, 1]], [[300.0, 20.0, 0.1]], periodic=True)
        rows = np.array([[0, 1, -1, -1]], dtype=np.int32)
        with pytest.raises(B.HipError, match='stack underflow'):
            ctx.term_expr_create(B.TERM_BOND, [X.OPCODES['ADD']], [], [], rows, np.zeros((0, 1)))
        with pytest.raises(B.HipError, match='is not a term-expression op'):
            ctx.term_expr_create(B.TERM_BOND, [X.PAIR_OPCODES['PAIR_R']], [], [], rows, np.zeros((0, 1)))
        with pytest.raises(B.HipError, match='variable index out of range'):
            ctx.term_expr_create(B.TERM_BOND, [X.TERM_OPCODES['TERM_VAR'] | (1 << 8)], [], [], rows, np.zeros((0, 1)))
        with pytest.raises(B.HipError, match='per-term parameter index out of range'):
            ctx.term_expr_create(B.TERM_BOND, [X.TERM_OPCODES['TERM_P'] | (2 << 8)], [], [], rows, np.ones((2, 1)))
        with pytest.raises(B.HipError, match='reads 0 globals'):
            ctx.term_expr_set_globals(fid, [1.0])
        with pytest.raises(B.HipError, match='1 terms of 3 parameters'):
            ctx.term_expr_set_params(fid, np.ones((2, 1)), 1)
        ctx.term_expr_release(fid)
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, np.zeros((3, 3)))
        ctx.check()
    finally:
        ctx.close()
        nobox.close()
