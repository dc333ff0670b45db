"""GPU tests of CustomGBForce (csrc/custom_gb.hip) against the fp64 torch restatements of its two test models on the CPU
(tests/custom_gb_cases.py, forces by autograd), through the C-ABI and through the AtomsMM-shaped API.

Tolerances are the project's own (tests/test_gpu_gb.py): energies rel 1e-10, forces 1e-9 of max|F|, computed
values rel 1e-12.  Shapes: n = 1 (no pair: the single-particle values and terms alone), n = 2 (one pair, also excluded), N5 (every
branch of the HCT integral, one atom outside a 1.0 nm cutoff), 257 atoms (one tile plus one atom) at 1 and at 64 lanes per row, S33 and
D1527 at the automatic width, each with NoCutoff and with a cutoff.  Every test prints what it measured.

Worst deviations measured on an MI355X: energy rel 6.9e-15, forces 4.0e-15 of max|F|, computed values rel 6.1e-14;
obc2-text against the hand-written GBSAOBCForce kernels energy rel 4.0e-15, forces 3.9e-15 of max|F|; 20 Verlet steps against them
max|dx| 0 nm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402
from atomsmm_amd.utils import InputError  # noqa: E402
import custom_gb_cases as M  # noqa: E402
import gb_cases as G  # noqa: E402

E_REL, F_REL, V_REL = 1e-10, 1e-9, 1e-12


@pytest.fixture(scope='module')
def cases(heaq, spcfw):
    water = G.with_radii(G.d1527(spcfw))
    return {'n1': G.tiny(1), 'n2': G.tiny(2), 'N5': G.n5(), 'S33': G.with_radii(G.s33(heaq)), 'D1527': water,
            'W257': {key: value[:257] for key, value in water.items()}}


@pytest.fixture(scope='module')
def references(cases):
    """The restatement per (model, case, cutoff), computed once and never written to."""
    table = {}

    def get(model, case, rc):
        if (model, case, rc) not in table:
            out = M.MODELS[model][1](cases[case], rc)
            for key in ('forces', 'values'):
                out[key].setflags(write=False)
            table[(model, case, rc)] = out
        return table[(model, case, rc)]
    return get


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, pos, f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def values_deviation(values, want):
    """The largest relative deviation; where the restatement gives an exact zero (a sum over no pairs) the kernel must, too."""
    zero = want == 0.0
    assert not values[zero].any()
    return float(np.abs(values[~zero] / want[~zero] - 1).max()) if (~zero).any() else 0.0


def assert_close(e, f, ref, what, values=None):
    scale = np.abs(ref['forces']).max()
    line = '%s: E = %.15g (restatement %.15g, rel %.2e)  max|dF| = %.3e of max|F| = %.6g' % (
        what, e, ref['energy'], abs(e - ref['energy']) / abs(ref['energy']), np.abs(f - ref['forces']).max(), scale)
    if values is not None:
        line += '  values rel %.2e' % values_deviation(values, ref['values'])
    print(line)
    assert e == pytest.approx(ref['energy'], rel=E_REL)
    if scale == 0.0:
        assert not f.any()                       # one atom: zeros, not small numbers
    else:
        assert np.abs(f - ref['forces']).max() <= F_REL * scale
    if values is not None:
        assert values_deviation(values, ref['values']) <= V_REL


# ------------------------------------------------------------------------------------ 1. the C-ABI against the restatements
@pytest.mark.parametrize('rc', [None, 1.0])
@pytest.mark.parametrize('case', ['n1', 'n2', 'N5', 'S33', 'D1527'])
@pytest.mark.parametrize('model', ['obc2-text', 'chain-table'])
def test_abi_parity(cases, references, model, case, rc):
    c = cases[case]
    n = len(c['positions'])
    ref = references(model, case, rc)
    force = M.MODELS[model][0](c, rc)
    ctx = B.HipContext(n, None)                  # no periodic box at all
    try:
        fid = M.create_on(ctx, force)
        pos = dev(c['positions'])
        values = ctx.custom_gb_values(fid, pos, force.getNumComputedValues())
        e, f = evaluate(ctx, fid, pos)
        assert_close(e, f, ref, '%s / %s / rc %s' % (model, case, rc), values)
        # no text reads x, y, z: the rows sum to zero
        if n > 1:
            assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()
        # accumulate: the rows are added to what the buffer holds, the energy to what the scalar holds
        start = np.random.default_rng(5).normal(size=(n, 3))
        e2, f2 = evaluate(ctx, fid, pos, accumulate=True, start=start)
        assert e2 == e and np.array_equal(f2, start + f)
        # the same positions again: the same bits
        e3, f3 = evaluate(ctx, fid, pos)
        assert e3 == e and np.array_equal(f3, f)
        # force only (no energy): the rows of the energy-carrying launch
        _, only = evaluate(ctx, fid, pos, energy=False)
        assert np.array_equal(only, f)
        assert np.array_equal(ctx.custom_gb_values(fid, pos, force.getNumComputedValues()), values)
        ctx.check()
    finally:
        ctx.close()


def test_one_excluded_pair(cases):
    """n = 2 with the pair excluded: V is zero, the ParticlePair term is gone, the ParticlePairNoExclusions term stays."""
    c = cases['n2']
    ctx = B.HipContext(2, None)
    try:
        results = {}
        for excl in ([], [(0, 1)]):
            ref = M.chain_reference(c, None, exclusions=excl)
            fid = M.create_on(ctx, M.chain_force(c, None, exclusions=excl))
            pos = dev(c['positions'])
            values = ctx.custom_gb_values(fid, pos, 3)
            e, f = evaluate(ctx, fid, pos)
            assert_close(e, f, ref, 'chain-table / n2 / exclusions %s' % excl, values if not excl else None)
            results[bool(excl)] = (e, values)
        assert not results[True][1][0].any() and results[False][1][0].all()
        assert results[True][0] != results[False][0]
        ctx.check()
    finally:
        ctx.close()


@pytest.mark.parametrize('model', ['obc2-text', 'chain-table'])
@pytest.mark.parametrize('width', [1, 64])
def test_one_tile_plus_one_atom(cases, references, model, width):
    c = cases['W257']
    ref = references(model, 'W257', 1.0)
    force = M.MODELS[model][0](c, 1.0)
    ctx = B.HipContext(257, None)
    try:
        ctx.set_option('cgb_lanes_per_row', width)
        fid = M.create_on(ctx, force)
        pos = dev(c['positions'])
        values = ctx.custom_gb_values(fid, pos, force.getNumComputedValues())
        e, f = evaluate(ctx, fid, pos)
        assert_close(e, f, ref, '%s / 257 atoms / %d lanes per row' % (model, width), values)
        ctx.check()
    finally:
        ctx.close()


def test_the_width_option_is_checked():
    ctx = B.HipContext(4, None)
    try:
        for bad in (3, 128, -1):
            with pytest.raises(B.HipError, match='cgb_lanes_per_row is 0 .automatic. or a power of two up to 64'):
                ctx.set_option('cgb_lanes_per_row', bad)
    finally:
        ctx.close()


@pytest.mark.parametrize('model', ['obc2-text', 'chain-table'])
def test_a_pair_at_the_cutoff(cases, model):
    """r < rc is the predicate: at rc = r (1 + 1e-9) the pair is inside, at rc = r (1 - 1e-9) outside."""
    c = cases['n2']
    r = float(np.linalg.norm(c['positions'][0] - c['positions'][1]))
    ctx = B.HipContext(2, None)
    try:
        energies = []
        for rc in (r * (1 + 1e-9), r * (1 - 1e-9)):
            ref = M.MODELS[model][1](c, rc)
            e, f = evaluate(ctx, M.create_on(ctx, M.MODELS[model][0](c, rc)), dev(c['positions']))
            assert_close(e, f, ref, '%s / n2 / rc = r (1 %+.0e)' % (model, rc / r - 1))
            energies.append(e)
            assert bool(f.any()) == (rc > r)
        assert energies[0] != energies[1]
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 2. two independent kernels
@pytest.mark.parametrize('rc', [None, 1.0])
@pytest.mark.parametrize('case', ['N5', 'S33', 'D1527'])
def test_obc2_text_against_the_hand_written_kernel(cases, case, rc):
    c = cases[case]
    ctx = B.HipContext(len(c['positions']), None)
    try:
        pos = dev(c['positions'])
        fid = M.create_on(ctx, M.obc2_force(c, rc))
        e_text, f_text = evaluate(ctx, fid, pos)
        gid = ctx.gb_create(c['charge'], c['radius'], c['scale'], rc=rc or 0.0)
        e_hand, f_hand = evaluate(ctx, gid, pos)
        scale = np.abs(f_hand).max()
        print('%s / rc %s: text %.15g, hand-written %.15g (rel %.2e), max|dF| = %.3e of %.6g' %
              (case, rc, e_text, e_hand, abs(e_text / e_hand - 1), np.abs(f_text - f_hand).max(), scale))
        assert e_text == pytest.approx(e_hand, rel=E_REL)
        assert np.abs(f_text - f_hand).max() <= F_REL * scale
        born = ctx.custom_gb_values(fid, pos, 2)[1]
        assert np.abs(born / ctx.gb_born_radii(gid, pos) - 1).max() <= V_REL
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 3. new numbers, same positions
def test_globals_parameters_and_tables_follow(cases):
    c = cases['S33']
    ctx = B.HipContext(33, None)
    try:
        force = M.chain_force(c, 1.0)
        fid = M.create_on(ctx, force)
        pos = dev(c['positions'])
        e0, _ = evaluate(ctx, fid, pos)
        # a global
        ctx.custom_gb_set_globals(fid, [0.4, 1.9])
        ref = M.chain_reference(c, 1.0, kappa=0.4, eps0=1.9)
        e1, f1 = evaluate(ctx, fid, pos)
        assert abs(e1 - e0) > 1e-3 * abs(e0)
        assert_close(e1, f1, ref, 'chain-table / S33 / kappa 0.4, eps0 1.9', ctx.custom_gb_values(fid, pos, 3))
        # the per-particle parameters
        par = M.chain_parameters(c)
        par[:, 1] *= 1.2
        par[:, 2] *= -0.5
        par[:, 0] = (par[:, 0] + 1) % 3
        ctx.custom_gb_set_params(fid, np.ascontiguousarray(par.T))
        ref = M.chain_reference(c, 1.0, kappa=0.4, eps0=1.9, parameters=par)
        e2, f2 = evaluate(ctx, fid, pos)
        assert abs(e2 - e1) > 1e-3 * abs(e1)
        assert_close(e2, f2, ref, 'chain-table / S33 / new parameters', ctx.custom_gb_values(fid, pos, 3))
        # the tables' values
        w = [1.3 * v + 0.1 * k for k, v in enumerate(M.W_VALUES)]
        s = [v * (1.0 + 0.05 * np.cos(k)) for k, v in enumerate(M.S_VALUES)]
        force.getTabulatedFunction(0).setFunctionParameters(3, 3, w)
        force.getTabulatedFunction(1).setFunctionParameters(s, M.S_LO, M.S_HI)
        from atomsmm_amd import tables as T
        ctx.custom_gb_set_tables(fid, [T.device_table(fn) for _, fn in force._functions])
        ref = M.chain_reference(c, 1.0, kappa=0.4, eps0=1.9, parameters=par, w_values=w, s_values=s)
        e3, f3 = evaluate(ctx, fid, pos)
        assert abs(e3 - e2) > 1e-3 * abs(e2)
        assert_close(e3, f3, ref, 'chain-table / S33 / new table values', ctx.custom_gb_values(fid, pos, 3))
        # sizes cannot change
        with pytest.raises(B.HipError, match='amm_custom_gb_set_tables: table 0 changed its kind or size'):
            ctx.custom_gb_set_tables(fid, [T.device_table(openmm.Discrete2DFunction(2, 2, [1.0] * 4)), T.device_table(force.getTabulatedFunction(1))])
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 4. in a Context
def solute_system(raw, force, group):
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    force.setForceGroup(group)
    system.addForce(force)
    return system


def test_get_state_separates_the_force_and_parameters_follow(cases, heaq):
    raw = G.s33(heaq)
    c = cases['S33']
    force = M.chain_force(c)
    system = solute_system(raw, force, 5)
    context = openmm.Context(system, openmm.VerletIntegrator(0.0))
    assert context._engine.free_space
    context.setPositions(raw['positions'] * unit.nanometers)

    def group5():
        state = context.getState(getEnergy=True, getForces=True, groups={5})
        return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value
    ref = M.chain_reference(c)
    e, f = group5()
    assert_close(e, f, ref, 'Context / chain-table / group 5', np.asarray(force.getComputedValues(context)))
    everything = context.getState(getEnergy=True, getForces=True)
    others = context.getState(getEnergy=True, getForces=True, groups={0})
    assert everything.getPotentialEnergy()._value == pytest.approx(others.getPotentialEnergy()._value + e, rel=E_REL)
    total = others.getForces(asNumpy=True)._value + f
    assert np.abs(everything.getForces(asNumpy=True)._value - total).max() <= F_REL * np.abs(total).max()
    # setParameter on a global
    context.setParameter('kappa', 0.45)
    e, f = group5()
    assert_close(e, f, M.chain_reference(c, kappa=0.45), 'Context / kappa 0.45')
    # updateParametersInContext on parameters and on table values
    par = M.chain_parameters(c)
    par[:, 1] *= 0.9
    for k in range(33):
        force.setParticleParameters(k, list(par[k]))
    w = [v + 0.25 for v in M.W_VALUES]
    force.getTabulatedFunction(0).setFunctionParameters(3, 3, w)
    force.updateParametersInContext(context)
    e, f = group5()
    assert_close(e, f, M.chain_reference(c, kappa=0.45, parameters=par, w_values=w), 'Context / new parameters and table')
    context._engine.ctx.check()


def test_twenty_verlet_steps_follow_the_hand_written_kernel(cases, heaq):
    """20 steps of VerletIntegrator(1 fs) with obc2-text against the same steps with GBSAOBCForce: two kernels that round differently;
    the bar is the 1e-9 nm of test_gpu_pair_expr.py for such a pair."""
    raw = G.s33(heaq)
    c = cases['S33']
    contexts, integrators = [], []
    for text in (False, True):
        if text:
            force = M.obc2_force(c)
        else:
            force = openmm.GBSAOBCForce()
            for q, r, s in zip(c['charge'], c['radius'], c['scale']):
                force.addParticle(float(q), float(r), float(s))
        integrators.append(openmm.VerletIntegrator(0.001))
        context = openmm.Context(solute_system(raw, force, 1), integrators[-1])
        context.setPositions(raw['positions'] * unit.nanometers)
        contexts.append(context)
    assert [sum(e.custom_gb is not None for e in k._engine.entries) for k in contexts] == [0, 1]
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
    moved = float(np.abs(xs[0] - raw['positions']).max())
    print('20 Verlet steps: max |x_text - x_hand-written| = %.3e nm (first above 1e-12 at step %s), atoms moved up to %.3e nm' % (worst, first, moved))
    assert moved > 1e-3
    assert worst <= 1e-9, 'measured %.3e nm, first above 1e-12 nm at step %s' % (worst, first)
    for context in contexts:
        context._engine.ctx.check()


def test_minimize_energy(cases, heaq):
    raw = G.s33(heaq)
    c = cases['S33']
    system = solute_system(raw, M.obc2_force(c), 1)
    simulation = app.Simulation(app.Topology(33), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(raw['positions'] * unit.nanometers)
    e0 = simulation.context.getState(getEnergy=True).getPotentialEnergy()._value
    info = simulation.context._engine.minimize(10.0, 50, None)
    e1 = simulation.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('minimize S33 + obc2-text: %.6f -> %.6f kJ/mol in %d iterations (%s)' % (e0, e1, info['iterations'], info['reason']))
    assert e1 < e0 and e1 == pytest.approx(info['energy'], rel=1e-9)
    x = simulation.context.getState(getPositions=True).getPositions(asNumpy=True)._value
    gb_only = simulation.context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value
    assert gb_only == pytest.approx(G.evaluate(dict(c, positions=x), None, want_forces=False)['energy'], rel=E_REL)
    simulation.minimizeEnergy(maxIterations=5)           # the public entry point
    assert simulation.context.getState(getEnergy=True).getPotentialEnergy()._value <= e1 + 1e-9 * abs(e1)
    simulation.context._engine.ctx.check()


def test_respa_with_the_force_in_the_outer_group(cases, heaq):
    raw = G.s33(heaq)
    system = solute_system(raw, M.chain_force(cases['S33']), 1)
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(system, integrator)
    context.setPositions(raw['positions'] * unit.nanometers)
    context.setVelocitiesToTemperature(300 * unit.kelvin, 1)
    integrator.step(5)
    state = context.getState(getPositions=True, getEnergy=True)
    x = state.getPositions(asNumpy=True)._value
    assert np.isfinite(x).all() and np.isfinite(state.getPotentialEnergy()._value) and np.abs(x - raw['positions']).max() > 1e-4
    context._engine.ctx.check()


def test_virtual_sites_spread_the_force(cases):
    """Atom 3 of N5 as the average of atoms 0 and 2: placed by the Context, its row spread to the parents."""
    c = cases['N5']
    system = openmm.System()
    for k, m in enumerate(c['mass']):
        system.addParticle(0.0 if k == 3 else float(m))
    system.setVirtualSite(3, openmm.TwoParticleAverageSite(0, 2, 0.4, 0.6))
    system.addForce(M.obc2_force(c))
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    context.setPositions(c['positions'] * unit.nanometers)
    context.computeVirtualSites()
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    assert np.allclose(x[3], 0.4 * x[0] + 0.6 * x[2], rtol=0, atol=1e-15)
    ref = G.evaluate(dict(c, positions=x))
    want = ref['forces'].copy()
    want[0] += 0.4 * want[3]
    want[2] += 0.6 * want[3]
    want[3] = 0.0
    state = context.getState(getEnergy=True, getForces=True)
    f = state.getForces(asNumpy=True)._value
    print('virtual site: E rel %.2e, max|dF| = %.3e of %.6g' % (abs(state.getPotentialEnergy()._value / ref['energy'] - 1), np.abs(f - want).max(), np.abs(want).max()))
    assert state.getPotentialEnergy()._value == pytest.approx(ref['energy'], rel=E_REL)
    assert np.abs(f - want).max() <= F_REL * np.abs(want).max()
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 5. refusals only the library can see
def test_the_library_refuses(cases):
    c = cases['N5']
    ctx = B.HipContext(5, None)
    try:
        force = M.obc2_force(c)
        progs = M.compiled(force)
        programs = [(p.code, p.consts) for p in progs.programs]
        params = np.ascontiguousarray(np.array(force._particles).T)
        glob = [78.3, 1.0]
        # a pair-type value behind the first
        with pytest.raises(B.HipError, match='computed value 1 is of a pair type: only the first'):
            ctx.custom_gb_create(2, [2, 2, 0, 0, 2], programs, glob, params)
        # a leaf outside its place: the Born radius program (it reads value 0) as value 0
        with pytest.raises(B.HipError, match='computed value 0 reads variable 1, which its place does not have'):
            ctx.custom_gb_create(2, [0, 0, 0, 0, 2], [programs[1], programs[1]] + programs[2:], glob, params)
        # a parameter the force does not have
        with pytest.raises(B.HipError, match='computed value 0 reads per-particle parameter 10 .the force has 1.'):       # sr2
            ctx.custom_gb_create(2, progs.types, programs, glob, params[:1])
        # too many of anything
        with pytest.raises(B.HipError, match='5 computed values .limit 4.'):
            ctx.custom_gb_create(5, [0] * 5, [programs[2]] * 5, glob, params)
        with pytest.raises(B.HipError, match='9 energy terms .limit 8.'):
            ctx.custom_gb_create(0, [0] * 9, [programs[2]] * 9, glob, params)
        with pytest.raises(B.HipError, match='9 per-particle parameters .limit 8.'):
            ctx.custom_gb_create(2, progs.types, programs, glob, np.zeros((9, 5)))
        # an exclusion that names no pair
        with pytest.raises(B.HipError, match=r'exclusion 0 \(1, 7\) names no pair'):
            ctx.custom_gb_create(2, progs.types, programs, glob, params, [(1, 7)])
        # wrong counts afterwards
        fid = M.create_on(ctx, force)
        with pytest.raises(B.HipError, match='the force reads 2 globals, 1 given'):
            ctx.custom_gb_set_globals(fid, [1.0])
        with pytest.raises(B.HipError, match='the force has 5 particles of 3 parameters, 5 x 2 given'):
            ctx.custom_gb_set_params(fid, params[:2])
        # tables that the programs read and nobody set; a table of the wrong kind
        chain = M.chain_force(c)
        cp = M.compiled(chain)
        cid = ctx.custom_gb_create(3, cp.types, [(p.code, p.consts) for p in cp.programs], [M.KAPPA, M.EPS0], np.ascontiguousarray(M.chain_parameters(c).T))
        pos = dev(c['positions'])
        with pytest.raises(B.HipError, match='the programs read tabulated functions and none are set'):
            evaluate(ctx, cid, pos)
        from atomsmm_amd import tables as T
        both = [T.device_table(fn) for _, fn in chain._functions]
        with pytest.raises(B.HipError, match='table 0 is of kind 0, the word that reads it takes kind 2'):
            ctx.custom_gb_set_tables(cid, both[::-1])
        with pytest.raises(B.HipError, match='a program reads table 1: 1 given'):
            ctx.custom_gb_set_tables(cid, both[:1])
        # the other families' entry points name this one, and this one's name the others
        gid = ctx.gb_create(c['charge'], c['radius'], c['scale'])
        with pytest.raises(B.HipError, match='not the id of a custom generalized-Born force .AMM_FORCE_CUSTOM_GB.: force %d is a generalized-Born force' % gid):
            ctx.custom_gb_values(gid, pos, 2)
        with pytest.raises(B.HipError, match='is a custom generalized-Born force .AMM_FORCE_CUSTOM_GB: amm_custom_gb_..'):
            ctx.gb_born_radii(fid, pos)
        e, _ = evaluate(ctx, fid, pos)                        # the refused calls changed nothing
        assert e == pytest.approx(G.evaluate(c)['energy'], rel=E_REL)
        ctx.custom_gb_release(fid)
        with pytest.raises(B.HipError, match='released'):
            evaluate(ctx, fid, pos)
        ctx.check()
    finally:
        ctx.close()


def test_the_size_limit_is_named():
    n = 32769
    ctx = B.HipContext(n, None)
    try:
        progs = M.compiled(M.obc2_force(G.tiny(1)))
        with pytest.raises(B.HipError, match='at most 32768 atoms'):
            ctx.custom_gb_create(2, progs.types, [(p.code, p.consts) for p in progs.programs], [78.3, 1.0], np.zeros((3, n)))       # nothing is evaluated
    finally:
        ctx.close()


def test_the_engine_refuses_on_the_gpu_path_as_on_the_host(cases, heaq):
    raw = G.s33(heaq)
    c = cases['S33']
    force = M.obc2_force(c)
    force.setNonbondedMethod(force.CutoffPeriodic)
    with pytest.raises(InputError, match='CustomGBForce: CutoffPeriodic is not supported'):
        openmm.Context(solute_system(raw, force, 1), openmm.VerletIntegrator(0.001))
    force = M.obc2_force(c)
    force.addEnergyTerm('q1*B2/r', force.ParticlePair)
    with pytest.raises(InputError, match='is not symmetric in particles 1 and 2'):
        openmm.Context(solute_system(raw, force, 1), openmm.VerletIntegrator(0.001))
    # a parameter the library refuses at updateParametersInContext: named, and the Context keeps its parameters
    force = M.obc2_force(c)
    context = openmm.Context(solute_system(raw, force, 1), openmm.VerletIntegrator(0.001))
    context.setPositions(raw['positions'] * unit.nanometers)
    e0 = context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value
    force.setParticleParameters(0, [float('nan'), 0.1, 0.1])
    with pytest.raises(InputError, match='CustomGBForce: amm_custom_gb_set_params: particle 0: a parameter is not finite'):
        force.updateParametersInContext(context)
    assert context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value == e0
    context._engine.ctx.check()
