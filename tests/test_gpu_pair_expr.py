"""GPU tests of the generic pair-expression force (csrc/pair_expr.hip): a CustomNonbondedForce whose energy text is none of the
hand-written families, compiled on the host and interpreted per pair.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 max|F|.  References: the CPU oracle of the
corresponding descriptor for texts that restate a hand-written family, tests/pair_expr_cases.py (mpmath radial functions, fp64 O(N^2)
sum) for texts no family covers, closed forms for the smallest shapes.

Worst deviations measured on an MI355X: rewritten families -- energy rel 2.5e-13, forces 6.1e-13 of max|F| (both the
force-switch text; the others 2.2e-14 and 8.4e-15); texts no family covers -- energy rel 1.6e-15, forces 8.3e-15 of max|F|; 20 Verlet
steps against the recognised force: 9.3e-15 nm."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import pair_expr_cases as P  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.forces import _near_terms, describe_energy  # noqa: E402
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
def custom_system(data, text, names, params, globals_, rc, rswitch=None, masses=None):
    """A System that holds ONE force: CustomNonbondedForce(text), CutoffPeriodic, raw per-particle parameters, the fixture's exclusions."""
    n = len(data['positions'])
    system = openmm.System()
    for m in (data['mass'] if masses is None else masses):
        system.addParticle(float(m))
    L = data['box']
    system.setDefaultPeriodicBoxVectors((float(L[0]), 0, 0), (0, float(L[1]), 0), (0, 0, float(L[2])))
    force = openmm.CustomNonbondedForce(text)
    for name in names:
        force.addPerParticleParameter(name)
    for name, value in globals_.items():
        force.addGlobalParameter(name, value)
    params = np.asarray(params, dtype=np.float64).reshape(n, len(names))
    for row in params:
        force.addParticle([float(v) for v in row])
    for i, j in data['exc_pairs']:
        force.addExclusion(int(i), int(j))
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(rc)
    if rswitch is not None:
        force.setUseSwitchingFunction(True)
        force.setSwitchingDistance(rswitch)
    system.addForce(force)
    return system, force


def context_with(system, data):
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(data['positions'] * unit.nanometers)
    return context


def energy_forces(context):
    state = context.getState(getEnergy=True, getForces=True)
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def generic_entry(context):
    (entry,) = [e for e in context._engine.entries if e.pair_expr]
    return entry


# ------------------------------------------------------------------------------------ 1. fails without the feature
def test_buckingham_text_runs_in_a_context(spcfw):
    """On the parent commit: InputError('energy expression not recognised by the HIP path ...')."""
    case = P.TEXTS['buckingham']
    params = P.typed_parameters(case, np.rint(spcfw['mass']), P.SEED)
    system, force = custom_system(spcfw, case['text'], case['names'], params, case['globals'], P.CUTOFF['spcfw'])
    assert describe_energy(force.getEnergyFunction(), {}) is None
    context = context_with(system, spcfw)
    e, f = energy_forces(context)
    entry = generic_entry(context)
    assert entry.pair_expr and len(entry.program.code) == 28
    assert math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1.0
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()          # every pair from both rows: the rows add up to nothing
    assert context._engine.ctx.pair_stats(entry.pair_ids[0])['list_kind'] == 0
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 2. the hand-written families, rewritten
KC = P.KC


def _rewritten(terms, extra=()):
    """The family's own text with its head wrapped so that describe_energy no longer knows it, and explicit mixing rules."""
    return ';'.join(['1*(%s)' % terms[0]] + list(terms[1:]) + list(extra) + [P.MIXING])


LJ = '4*epsilon*((sigma/r)^12 - (sigma/r)^6)'
FAMILY_CASES = {
    # name: (text, globals, cutoff, built-in switch, oracle descriptor, pairs within the cutoff)
    'near-none': (_rewritten(_near_terms(1.0, 0.8, None)), dict(Kc=KC, rc0=1.0, rs0=0.8), 1.0, None,
                  lambda: O.desc(O.NEAR_NONE, rc=1.0, rc0=1.0, rs0=0.8), 314034),
    'near-shift': (_rewritten(_near_terms(1.0, 0.8, 'shift')), dict(Kc=KC, rc0=1.0, rs0=0.8), 1.0, None,
                   lambda: O.desc(O.NEAR_SHIFT, rc=1.0, rc0=1.0, rs0=0.8), 314034),
    'damped-2': (_rewritten(['S*({} + erfc(alpha*r)*Kc*chargeprod/r)'.format(LJ), 'S = 1 + step(r - rswitch)*u^3*(15*u - 6*u^2 - 10)',
                             'u = (r^d - rswitch^d)/(rcut^d - rswitch^d)', 'd=2']), dict(Kc=KC, alpha=2.9, rswitch=0.9, rcut=1.0), 1.0, None,
                 lambda: O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=2), 314034),
    'ljc-switch': (_rewritten([LJ + ' + Kc*chargeprod/r']), dict(Kc=KC), 1.0, 0.9,
                   # (a CustomNonbondedForce's built-in switch multiplies the WHOLE energy -- a NonbondedForce's only its Lennard-Jones
                   # part: the descriptor that says the same is the damped family of degree 1 with alpha = 0, erfc(0) = 1)
                   lambda: O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=0.0, degree=1), 314034),
    'near-fswitch': (_rewritten(_near_terms(0.7, 0.5, 'force-switch')), dict(Kc=KC, rc0=0.7, rs0=0.5), 0.7, None,
                     lambda: O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5), 106161),
}


@pytest.mark.parametrize('name', sorted(FAMILY_CASES))
def test_rewritten_families_against_the_oracle(spcfw, name):
    text, globals_, rc, rswitch, desc, npairs = FAMILY_CASES[name]
    assert describe_energy(text, globals_) is None
    assert len(spcfw['positions']) == 1536 and spcfw['box'][0] == 2.5
    params = np.stack([spcfw['charge'], spcfw['sigma'], spcfw['epsilon']], axis=1)
    system, force = custom_system(spcfw, text, ['charge', 'sigma', 'epsilon'], params, globals_, rc, rswitch)
    context = context_with(system, spcfw)
    e, f = energy_forces(context)
    entry = generic_entry(context)
    engine = context._engine
    # the input checks itself
    assert engine.ctx.pair_count_within(entry.pair_ids[0], engine.x, rc) // 2 == npairs
    assert engine.ctx.pair_stats(entry.pair_ids[0])['list_kind'] == 0
    e_ref, f_ref, counted = O.pair_eval(desc(), spcfw['positions'], spcfw['box'], spcfw['charge'], spcfw['sigma'], spcfw['epsilon'],
                                        spcfw['exc_pairs'])
    assert counted == npairs
    b = 0.5 / (0.7 - 0.5)          # force-switch: the energy bar is 1e-8 only where b = rs / (rc - rs) >~ 10 (golden G3's conditioning)
    assert_close(e, f, e_ref, f_ref, 'q-SPC-FW / %s (%d code words)' % (name, len(entry.program.code)),
                 e_rel=1e-8 if (name == 'near-fswitch' and b >= 10) else E_REL)
    engine.ctx.check()


# ------------------------------------------------------------------------------------ 3. texts no family covers
@pytest.fixture(scope='module')
def references():
    """(energy, forces, tables) of tests/pair_expr_cases.py per (fixture, text), computed once and never written to."""
    made = {}

    def get(fixture, name, data, params):
        if (fixture, name) not in made:
            tables = {}
            e, f = P.pair_sum(P.TEXTS[name], params, data['positions'], data['box'], P.CUTOFF[fixture], data['exc_pairs'], tables=tables)
            f.setflags(write=False)
            made[(fixture, name)] = (e, f, tables)
        return made[(fixture, name)]
    return get


@pytest.mark.parametrize('fixture,name', P.GPU_CASES)
def test_texts_no_family_covers(request, references, fixture, name):
    data = request.getfixturevalue(fixture)
    if fixture == 'heaq':
        assert len(data['positions']) == 1083 and abs(data['box'][0] - 2.1787) < 1e-12
    case = P.TEXTS[name]
    params = P.typed_parameters(case, np.rint(data['mass']), P.SEED)          # one row per element: every slot differs between types
    system, force = custom_system(data, case['text'], case['names'], params, case['globals'], P.CUTOFF[fixture])
    assert describe_energy(case['text'], case['globals']) is None
    context = context_with(system, data)
    e, f = energy_forces(context)
    e_ref, f_ref, _ = references(fixture, name, data, params)
    assert_close(e, f, e_ref, f_ref, '%s / %s' % (fixture, name))
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 4. the smallest shapes, at the C-ABI
YUKAWA = 'q1*q2*exp(-b*r)/r'


def yukawa(r, qq, b):
    """(E, dE/dr) in closed form."""
    e = qq * math.exp(-b * r) / r
    return e, -e * (b + 1.0 / r)


def abi_force(ctx, params, excl=None, rc=0.9, rswitch=None, b=2.5, skin=-1.0):
    prog = X.compile_pair(YUKAWA, ['q'], ['b'])
    desc = B.pair_desc(B.PAIR_EXPR, rc, rswitch=rswitch or 0.0, flags=B.SWITCH if rswitch else 0)
    return ctx.pair_expr_create(desc, prog.code, prog.consts, [b], params, None, None, excl, skin=skin)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


BOX = np.full(3, 4.0)


def test_one_atom_gives_zeros():
    ctx = B.HipContext(1, BOX)
    try:
        fid = abi_force(ctx, np.array([1.5]))
        e, f = evaluate(ctx, fid, np.array([[0.3, 0.4, 0.5]]))
        assert e == 0.0 and not f.any()          # zeros, not small numbers
        ctx.check()
    finally:
        ctx.close()


@pytest.mark.parametrize('case', ['across-a-face', 'excluded', 'inside-rc', 'outside-rc', 'in-the-switch'])
def test_two_atoms(case):
    q = np.array([1.5, -0.7])
    rc, b = 0.9, 2.5
    r = {'across-a-face': 0.15, 'excluded': 0.3, 'inside-rc': rc * (1 - 1e-9), 'outside-rc': rc * (1 + 1e-9), 'in-the-switch': 0.8}[case]
    if case == 'across-a-face':
        pos = np.array([[0.05, 1.0, 2.0], [BOX[0] - 0.10, 1.0, 2.0]])          # 3.85 nm apart in the box, 0.15 nm through its face
    else:
        pos = np.array([[1.0, 1.0, 2.0], [1.0 + r, 1.0, 2.0]])
    d = pos[0] - pos[1]
    d -= BOX * np.rint(d / BOX)
    r = float(np.sqrt(d @ d))
    ctx = B.HipContext(2, BOX)
    try:
        fid = abi_force(ctx, q, excl=np.array([[0, 1]], np.int32) if case == 'excluded' else None, rc=rc,
                        rswitch=0.7 if case == 'in-the-switch' else None, b=b)
        e, f = evaluate(ctx, fid, pos)
        if case in ('excluded', 'outside-rc'):
            assert e == 0.0 and not f.any()
            return
        e_ref, de_ref = yukawa(r, q[0] * q[1], b)
        if case == 'in-the-switch':
            t = (r - 0.7) / (rc - 0.7)
            s, ds = 1 - 10 * t ** 3 + 15 * t ** 4 - 6 * t ** 5, (-30 * t ** 2 + 60 * t ** 3 - 30 * t ** 4) / (rc - 0.7)
            e_ref, de_ref = s * e_ref, s * de_ref + ds * e_ref
        f_ref = np.stack([-de_ref * d / r, de_ref * d / r])
        assert_close(e, f, e_ref, f_ref, 'n = 2 / ' + case)
        ctx.check()
    finally:
        ctx.close()


def test_sixty_five_atoms_on_a_line():
    """65 rows (more than one wavefront of lanes), rows longer than the lanes that share them; accumulate onto a buffer that holds
    numbers; forces bit for bit the same with and without the energy."""
    n, b, rc = 65, 2.5, 0.9
    rng = np.random.default_rng(3)
    pos = np.stack([0.1 + 0.02 * np.arange(n) + rng.uniform(-0.002, 0.002, n), np.full(n, 1.0), np.full(n, 2.0)], axis=1)
    q = rng.uniform(0.5, 1.5, n)
    e_ref, f_ref = 0.0, np.zeros((n, 3))
    for i in range(n):
        for j in range(i + 1, n):
            d = pos[i] - pos[j]
            r = float(np.sqrt(d @ d))
            if r < rc:
                e, de = yukawa(r, q[i] * q[j], b)
                e_ref += e
                f_ref[i] -= de * d / r
                f_ref[j] += de * d / r
    ctx = B.HipContext(n, BOX)
    try:
        fid = abi_force(ctx, q, rc=rc, b=b)
        e, f = evaluate(ctx, fid, pos)
        assert_close(e, f, e_ref, f_ref, '65 on a line')
        st = ctx.pair_stats(fid)
        assert st['list_kind'] == 0 and st['max_neighbors'] > st['lanes_per_atom'] and n * st['lanes_per_atom'] > 64
        start = rng.normal(size=(n, 3))
        e2, f2 = evaluate(ctx, fid, pos, accumulate=True, start=start)
        assert e2 == e and np.array_equal(f2, start + f)
        _, f3 = evaluate(ctx, fid, pos, energy=False)
        assert np.array_equal(f3, f)
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 5. parameters follow
def test_globals_particle_parameters_and_the_box_follow(spcfw):
    case = P.TEXTS['gauss-coulomb']
    rc = P.CUTOFF['spcfw']
    params = P.typed_parameters(case, np.rint(spcfw['mass']), P.SEED)
    system, force = custom_system(spcfw, case['text'], case['names'], params, case['globals'], rc)
    context = context_with(system, spcfw)
    e0, _ = energy_forces(context)
    tables = {}

    def reference(params, box=spcfw['box'], **globals_):
        return P.pair_sum(case, params, spcfw['positions'], box, rc, spcfw['exc_pairs'], gvalues=dict(case['globals'], **globals_), tables=tables)
    # Context.setParameter of a global
    context.setParameter('beta', 2.0)
    e1, f1 = energy_forces(context)
    e_ref, f_ref = reference(params, beta=2.0)
    assert abs(e1 - e0) > 1e-3 * abs(e0)
    assert_close(e1, f1, e_ref, f_ref, 'beta = 2')
    # setParticleParameters + updateParametersInContext
    changed = params.copy()
    changed[7] = 1.75
    force.setParticleParameters(7, [1.75])
    force.updateParametersInContext(context)
    e2, f2 = energy_forces(context)
    e_ref, f_ref = reference(changed, beta=2.0)
    assert abs(e2 - e1) > 1e-6 * abs(e1)
    assert_close(e2, f2, e_ref, f_ref, 'q[7] = 1.75')
    # the box grows by 1 % (positions stay: the pairs through its faces change)
    grown = spcfw['box'] * 1.01
    context.setPeriodicBoxVectors((grown[0], 0, 0), (0, grown[1], 0), (0, 0, grown[2]))
    e3, f3 = energy_forces(context)
    e_ref, f_ref = reference(changed, box=grown, beta=2.0)
    assert abs(e3 - e2) > 1e-6 * abs(e2)
    assert_close(e3, f3, e_ref, f_ref, 'box + 1 %')
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 6. in a step program
def near_none_system(spcfw, generic, group=0):
    """Flexible q-SPC-FW whose only pair force is the near-none potential (rc0 = 1.0, rs0 = 0.8): the recognised NearNonbondedForce, or
    the same text rewritten so that it takes the pair-expression kernel."""
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic', cutoff=1.0)
    nb = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    if not generic:
        near = atomsmm.NearNonbondedForce(1.0 * unit.nanometers, 0.8 * unit.nanometers, None).importFrom(nb)
        near.setForceGroup(group)
        near.addTo(system)
        return system
    text, globals_, rc, _, _, _ = FAMILY_CASES['near-none']
    force = openmm.CustomNonbondedForce(text)
    for name in ('charge', 'sigma', 'epsilon'):
        force.addPerParticleParameter(name)
    for name, value in globals_.items():
        force.addGlobalParameter(name, value)
    for q, s, e in zip(spcfw['charge'], spcfw['sigma'], spcfw['epsilon']):
        force.addParticle([float(q), float(s), float(e)])
    for i, j in spcfw['exc_pairs']:
        force.addExclusion(int(i), int(j))
    force.setNonbondedMethod(force.CutoffPeriodic)
    force.setCutoffDistance(rc)
    force.setForceGroup(group)
    system.addForce(force)
    return system


def test_twenty_verlet_steps_follow_the_hand_written_kernel(spcfw):
    """20 steps of VerletIntegrator(1 fs): the two kernels round differently; positions agree to 1e-9 nm over this horizon."""
    contexts, integrators = [], []
    for generic in (False, True):
        integrators.append(openmm.VerletIntegrator(0.001))
        context = openmm.Context(near_none_system(spcfw, generic), integrators[-1])
        context.setPositions(spcfw['positions'] * unit.nanometers)
        contexts.append(context)
    assert [sum(e.pair_expr for e in c._engine.entries) for c in contexts] == [0, 1]
    first, worst = None, 0.0
    for step in range(1, 21):
        xs = []
        for context, integrator in zip(contexts, integrators):
            integrator.step(1)
            xs.append(context.getState(getPositions=True).getPositions(asNumpy=True)._value)
        diff = float(np.abs(xs[0] - xs[1]).max())
        worst = max(worst, diff)
        if first is None and diff > 1e-12:
            first = step
    moved = float(np.abs(xs[0] - spcfw['positions']).max())
    print('20 Verlet steps: max |x_generic - x_family| = %.3e nm (first above 1e-12 at step %s), atoms moved up to %.3e nm' % (worst, first, moved))
    assert moved > 1e-3
    assert worst <= 1e-9, 'measured %.3e nm, first above 1e-12 nm at step %s' % (worst, first)
    for context in contexts:
        context._engine.ctx.check()


def test_respa_program_with_the_generic_force_in_group_one(spcfw):
    system = near_none_system(spcfw, True, group=1)
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(system, integrator)
    context.setPositions(spcfw['positions'] * unit.nanometers)
    integrator.step(5)
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    assert np.isfinite(x).all() and np.abs(x - spcfw['positions']).max() > 1e-4
    assert generic_entry(context).group == 1
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 7. refusals at the ABI
def test_refusals_name_the_family():
    ctx = B.HipContext(2, BOX)
    try:
        q = np.array([1.0, 2.0])
        fid = abi_force(ctx, q)
        other = ctx.pair_create(B.pair_desc(B.NEAR_NONE, 1.0, rc0=1.0, rs0=0.8), q, q, q)
        out = torch.zeros(1, dtype=torch.float64, device='cuda')
        pos = dev(np.array([[1.0, 1.0, 1.0], [1.3, 1.0, 1.0]]))
        for call in (lambda: ctx.pair_share_list(fid, other), lambda: ctx.pair_share_list(other, fid),
                     lambda: ctx.pair_energy_derivative(fid, pos, out), lambda: ctx.pair_set_lambda(fid, 0.5),
                     lambda: ctx.pair_energy_states(fid, pos, out, out),
                     lambda: ctx.pair_create(B.pair_desc(B.PAIR_EXPR, 1.0), q, q, q)):
            with pytest.raises(B.HipError, match='AMM_PAIR_EXPR'):
                call()
        prog = X.compile_pair(YUKAWA, ['q'], ['b'])
        with pytest.raises(B.HipError, match='AMM_PAIR_EXPR.*AMM_FREE_SPACE'):
            ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, 0.9, flags=B.FREE_SPACE), prog.code, prog.consts, [2.5], q, None, None)
        with pytest.raises(B.HipError, match='reads 1 globals'):
            ctx.pair_expr_set_globals(fid, [1.0, 2.0])
        # a program that would leave the stack is refused on the host, before any launch
        with pytest.raises(B.HipError, match='stack underflow'):
            ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, 0.9), [X.OPCODES['ADD']], [], [], q, None, None)
        with pytest.raises(B.HipError, match='global index out of range'):
            ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, 0.9), [X.OPCODES['GLOBAL'] | (3 << 8)], [], [1.0], q, None, None)
        # set_params stores raw values (a negative third slot is a value like any other)
        ctx.pair_set_params(fid, np.array([2.0, -3.0]), np.array([0.0, 0.0]), np.array([-1.0, 0.0]))
        e, f = evaluate(ctx, fid, pos.cpu().numpy())
        e_ref, de_ref = yukawa(0.3, -6.0, 2.5)
        assert e == pytest.approx(e_ref, rel=E_REL) and f[0, 0] == pytest.approx(de_ref, rel=F_REL)
        ctx.check()
    finally:
        ctx.close()
