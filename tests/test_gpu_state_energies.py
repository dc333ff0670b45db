"""Energies at many global-parameter states in one pass (amm_pair_energy_states, Engine.energies_at_states) and the stale sorted
copies after amm_pair_set_params: the C-ABI against the CPU oracle and against the existing energy path, then the engine against
the set / evaluate / restore loop of the reference's reporters on a SolvationSystem (HEAQ, and config C5 at full size)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.testing import build_c5_system, solvated_chain, system_from_arrays  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def softcore(ctx, h, codes, lam=0.5):
    desc = B.pair_desc(B.SOFTCORE, 1.0, rswitch=0.9, alpha=lam, flags=B.SWITCH, Kc=1.0)
    return ctx.pair_create(desc, codes, h['sigma'], h['epsilon'], h['exc_pairs'])


def oracle_energy(h, codes, lam):
    d = O.desc(O.SOFTCORE, rc=1.0, rswitch=0.9, alpha=float(lam), flags=O.SWITCH, Kc=1.0)
    return O.pair_eval(d, h['positions'], h['box'], codes, h['sigma'], h['epsilon'], h['exc_pairs'])[0]


def energy_now(ctx, fid, pos, n):
    f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
    en = torch.zeros(1, dtype=torch.float64, device='cuda')
    ctx.force_eval(fid, pos, f, accumulate=False, energy=en)
    ctx.check()
    return en.item()


def states(ctx, fid, pos, lambdas):
    out = torch.zeros(len(lambdas), dtype=torch.float64, device='cuda')
    ctx.pair_energy_states(fid, pos, dev(lambdas), out)
    ctx.check()
    return out.cpu().numpy()


def lambda_table(K):
    return np.array([0.5]) if K == 1 else np.linspace(0.0, 1.0, K)


@pytest.mark.parametrize('K', [1, 7, 64])
def test_softcore_states_vs_oracle_and_energy_path(heaq, K):
    """One launch at K lambdas (0 and 1 among them) against the oracle and against the existing energy path at each lambda; a
    second launch gives the same bits; the force's own lambda is untouched."""
    h = heaq
    n = len(h['positions'])
    codes = np.where(h['resname'] == 'aaa', 1.0, 2.0)
    ctx = B.HipContext(n, h['box'])
    fid = softcore(ctx, h, codes, lam=0.35)
    pos = dev(h['positions'])
    own = energy_now(ctx, fid, pos, n)
    assert ctx.pair_stats(fid)['list_kind'] == 3                  # the list-free path
    lambdas = lambda_table(K)
    got = states(ctx, fid, pos, lambdas)
    again = states(ctx, fid, pos, lambdas)
    assert np.array_equal(got, again)
    checked = range(K) if K <= 7 else list(range(0, K, 9)) + [K - 1]
    for k in checked:
        assert got[k] == pytest.approx(oracle_energy(h, codes, lambdas[k]), rel=1e-10, abs=1e-12)
    for k, lam in enumerate(lambdas):
        ctx.pair_set_lambda(fid, lam)
        ref = energy_now(ctx, fid, pos, n)
        assert got[k] == pytest.approx(ref, rel=1e-11, abs=1e-12), (k, lam)
    assert got[0] == (0.0 if K > 1 else got[0])                    # lambda = 0: no coupling at all
    ctx.pair_set_lambda(fid, 0.35)
    assert energy_now(ctx, fid, pos, n) == own
    ctx.close()


def test_softcore_states_adds_and_leaves_a_device_lambda_bound(heaq):
    h = heaq
    n = len(h['positions'])
    codes = np.where(h['resname'] == 'aaa', 1.0, 2.0)
    ctx = B.HipContext(n, h['box'])
    fid = softcore(ctx, h, codes, lam=0.9)
    pos = dev(h['positions'])
    scal = dev([0.0, 0.25])
    ctx.pair_set_lambda_dev(fid, scal, 1)
    bound = energy_now(ctx, fid, pos, n)
    assert bound == pytest.approx(oracle_energy(h, codes, 0.25), rel=1e-10)
    lambdas = np.array([0.1, 0.6])
    out = dev([1.0, 2.0])                                          # (+=, not =)
    ctx.pair_energy_states(fid, pos, dev(lambdas), out)
    ctx.check()
    res = out.cpu().numpy()
    for k, lam in enumerate(lambdas):
        assert res[k] - (1.0 + k) == pytest.approx(oracle_energy(h, codes, lam), rel=1e-10)
    assert energy_now(ctx, fid, pos, n) == bound                     # still lambda = scalars[1]
    scal[1] = 0.7
    assert energy_now(ctx, fid, pos, n) == pytest.approx(oracle_energy(h, codes, 0.7), rel=1e-10)
    ctx.close()


def test_softcore_states_on_the_list_path(heaq):
    """Both sets large (no small set: the filtered neighbour list): K evaluations of the existing energy path inside the ABI."""
    h = heaq
    n = len(h['positions'])
    codes = np.where(np.arange(n) < n // 2, 1.0, 2.0)
    ctx = B.HipContext(n, h['box'])
    fid = softcore(ctx, h, codes, lam=0.4)
    pos = dev(h['positions'])
    own = energy_now(ctx, fid, pos, n)
    assert ctx.pair_stats(fid)['list_kind'] != 3
    lambdas = np.array([0.0, 0.3, 1.0])
    got = states(ctx, fid, pos, lambdas)
    for k, lam in enumerate(lambdas):
        assert got[k] == pytest.approx(oracle_energy(h, codes, lam), rel=1e-10, abs=1e-12)
    assert energy_now(ctx, fid, pos, n) == own
    ctx.close()


def test_pair_energy_states_rejects_bad_arguments(heaq):
    h = heaq
    n = len(h['positions'])
    codes = np.where(h['resname'] == 'aaa', 1.0, 2.0)
    ctx = B.HipContext(n, h['box'])
    fid = softcore(ctx, h, codes)
    pos = dev(h['positions'])
    for K in (0, B.MAX_STATES + 1):
        with pytest.raises(B.HipError, match='n_states'):
            ctx.pair_energy_states(fid, pos, torch.zeros(K, dtype=torch.float64, device='cuda'),
                                   torch.zeros(K, dtype=torch.float64, device='cuda'))
    with pytest.raises(B.HipError, match='invalid pair force id'):
        ctx.pair_energy_states(fid + 7, pos, dev([0.5]), dev([0.0]))
    lj = ctx.pair_create(B.pair_desc(B.NONBONDED, 1.0), h['charge'], h['sigma'], h['epsilon'], h['exc_pairs'])
    with pytest.raises(B.HipError, match='softcore'):
        ctx.pair_energy_states(lj, pos, dev([0.5]), dev([0.0]))
    ctx.close()


def test_set_params_invalidates_sorted_copies(spcfw):
    """positions_private with the bound positions: an evaluation, new charges (amm_pair_set_params), an evaluation at the SAME
    positions -- the second one must use the new charges, not the sorted copies the first one left."""
    c = spcfw
    n = len(c['positions'])
    d = O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5)
    ctx = B.HipContext(n, c['box'])
    ctx.set_option('positions_private', 1)
    desc = B.pair_desc(B.NEAR_FSWITCH, 0.7, rc0=0.7, rs0=0.5)
    fid = ctx.pair_create(desc, c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'], skin=0.1)
    x, v, m = dev(c['positions']), dev(np.zeros((n, 3))), dev(c['mass'])
    ctx.bind_state(x, v, m)
    for scale in (1.0, 0.5, 0.25):
        q = c['charge'] * scale
        if scale != 1.0:
            ctx.pair_set_params(fid, q, c['sigma'], c['epsilon'])
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        ctx.force_eval(fid, x, f)                                   # force only (the molecule-row traversal)
        en = torch.zeros(1, dtype=torch.float64, device='cuda')
        g = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        ctx.force_eval(fid, x, g, energy=en)
        ctx.check()
        e_ref, f_ref, _ = O.pair_eval(d, c['positions'], c['box'], q, c['sigma'], c['epsilon'], c['exc_pairs'])
        assert np.abs(f.cpu().numpy() - f_ref).max() <= 1e-9 * np.abs(f_ref).max(), scale
        assert np.abs(g.cpu().numpy() - f_ref).max() <= 1e-9 * np.abs(f_ref).max(), scale
        assert en.item() == pytest.approx(e_ref, rel=1e-10), scale
    ctx.close()


# ------------------------------------------------------------------------------------------------ engine
def reference_loop(context, names, rows):
    """The reference's reporters: set each state, getState(getEnergy=True), restore."""
    original = {name: context.getParameter(name) for name in names}
    latest = dict(original)
    out = []
    for row in rows:
        for name, value in zip(names, row):
            if value != latest[name]:
                context.setParameter(name, value)
                latest[name] = value
        out.append(context.getState(getEnergy=True).getPotentialEnergy()._value)
    for name, value in original.items():
        if value != latest[name]:
            context.setParameter(name, value)
    return np.array(out)


def tables():
    lam = np.linspace(0.0, 1.0, 11)
    return {'vdw': (['lambda_vdw'], lam[:, None]),
            'coul': (['lambda_coul'], lam[:, None]),
            'both': (['lambda_vdw', 'lambda_coul'], np.stack([lam, lam[::-1]], axis=1))}


def check_tables(context, expect_paths):
    eng = context._engine
    before = context.getState(getEnergy=True).getPotentialEnergy()._value
    params = dict(context.getParameters())
    for key, (names, rows) in tables().items():
        if key not in expect_paths:
            continue
        paths0, fallbacks0 = dict(eng.state_paths), eng.n_state_fallbacks
        got = eng.energies_at_states(names, rows)
        used = {p for p in eng.state_paths if eng.state_paths[p] > paths0[p]}
        assert used == expect_paths[key], (key, used)
        assert eng.n_state_fallbacks - fallbacks0 == (1 if 'loop' in used else 0)
        assert dict(context.getParameters()) == params
        ref = reference_loop(context, names, rows)
        scale = np.abs(ref).max()
        assert np.abs(got - ref).max() <= 1e-9 * scale, (key, got - ref)
    assert context.getState(getEnergy=True).getPotentialEnergy()._value == pytest.approx(before, rel=1e-12)


def heaq_context(heaq, use_softcore=True):
    system = system_from_arrays(heaq, nonbondedMethod='PME', cutoff=1.0, switch=0.9)
    solute = set(int(i) for i in np.where(heaq['resname'] == 'aaa')[0])
    solvation = atomsmm.SolvationSystem(system, solute, use_softcore=use_softcore)
    context = openmm.Context(solvation, openmm.VerletIntegrator(1 * unit.femtoseconds))
    context.setPositions(heaq['positions'] * unit.nanometers)
    context.setParameter('lambda_vdw', 0.6)
    context.setParameter('lambda_coul', 0.3)
    return context


def test_energies_at_states_heaq(heaq):
    """SolvationSystem (PME): lambda_vdw through the softcore states launch, lambda_coul by the exact quadratic of the charge
    offsets, both at once by the two together -- no reference loop."""
    context = heaq_context(heaq)
    check_tables(context, {'vdw': {'once', 'states'}, 'coul': {'once', 'quadratic'}, 'both': {'once', 'states', 'quadratic'}})


def test_energies_at_states_heaq_reference_loop(heaq):
    """use_softcore=False: lambda_vdw scales sigma / epsilon offsets of the NonbondedForce -- no shortcut, the reference loop."""
    context = heaq_context(heaq, use_softcore=False)
    check_tables(context, {'vdw': {'once', 'loop'}, 'coul': {'once', 'quadratic'}, 'both': {'once', 'loop'}})


def test_energies_at_states_c5_full_size():
    case = solvated_chain()
    respa = build_c5_system(case)
    context = openmm.Context(respa, openmm.VerletIntegrator(1 * unit.femtoseconds))
    context.setPositions(case['positions'] * unit.nanometers)
    context.setParameter('lambda_vdw', 0.6)
    eng = context._engine
    # (the synthetic solute carries no charge: C5 has no lambda_coul)
    assert 'lambda_coul' not in eng.parameters
    check_tables(context, {'vdw': {'once', 'states'}})


def _afed_simulation(case):
    from atomsmm_amd.openmm import app
    respa = build_c5_system(case)
    inner = atomsmm.RespaPropagator([2, 2, 1]).integrator(1 * unit.femtoseconds)
    var = atomsmm.ExtendedSystemVariable('lambda_vdw', 50, 2.5, 20 * unit.femtoseconds)
    integrator = atomsmm.AdiabaticDynamicsIntegrator(inner, 2, [var])
    integrator.setRandomNumberSeed(11)
    simulation = app.Simulation(app.Topology(len(case['positions'])), respa, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(case['positions'] * unit.nanometers)
    simulation.context.setVelocities(case['velocities'])
    simulation.context.setParameter('lambda_vdw', 0.8)
    return simulation


def test_state_reports_leave_an_afed_run_unchanged():
    """An AFED run on lambda_vdw with ExtendedStateDataReporter(globalParameterStates=...) every 2 steps ends in the same positions,
    velocities and lambda, bit for bit, as the same run without it; the reported energies are those of the reference loop."""
    import io
    import pandas as pd
    case = solvated_chain(nside=12, n_chain=300, n_solute=30)
    lam = np.linspace(0.0, 1.0, 6)
    table = pd.DataFrame({'lambda_vdw': lam})
    out = {}
    for with_reports in (False, True):
        simulation = _afed_simulation(case)
        text = io.StringIO()
        if with_reports:
            simulation.reporters.append(atomsmm.ExtendedStateDataReporter(text, 2, step=True, globalParameterStates=table,
                                                                          globalParameters=['lambda_vdw']))
        for _ in range(3):                  # (the same step() calls with and without reports: AFED settles its device scalars per call)
            simulation.step(2)
        st = simulation.context.getState(getPositions=True, getVelocities=True)
        out[with_reports] = (st.getPositions(asNumpy=True)._value, st.getVelocities(asNumpy=True)._value,
                             simulation.context.getParameter('lambda_vdw'), text.getvalue(), simulation)
    assert np.array_equal(out[True][0], out[False][0])
    assert np.array_equal(out[True][1], out[False][1])
    assert out[True][2] == out[False][2]
    lines = out[True][3].splitlines()
    assert lines[0] == '#"Step",' + ','.join('"Energy[{}] (kJ/mole)"'.format(k) for k in range(6)) + ',"lambda_vdw"'
    assert [int(line.split(',')[0]) for line in lines[1:]] == [2, 4, 6]
    last = np.array([float(v) for v in lines[-1].split(',')[1:7]])
    ref = reference_loop(out[True][4].context, ['lambda_vdw'], lam[:, None])
    assert np.abs(last - ref).max() <= 1e-9 * np.abs(ref).max()
    assert float(lines[-1].split(',')[-1]) == out[True][2]


def test_states_launch_walks_the_candidates():
    """Fused RESPA inner iterations keep the softcore force's candidate list (option group_candidates, as in test_gpu_c5); right after
    a step the states launch -- alone, and inside energies_at_states -- walks the candidates only (counted with the force's candidate
    walks) and gives the energies of the walk over every atom (group_candidates = 0) and of the energy path.  (A step may end in a
    rebuild of the companion list: the candidates then wait for the next fused iteration.)"""
    case = solvated_chain(nside=12, n_chain=300, n_solute=30)
    respa = build_c5_system(case)
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(2 * unit.femtoseconds)
    context = openmm.Context(respa, integrator)
    eng = context._engine
    eng.ctx.set_option('group_candidates', 1)
    eng.ctx.set_option('terms_from', 1)
    context.setPositions(case['positions'] * unit.nanometers)
    context.setVelocities(case['velocities'])
    context.setParameter('lambda_vdw', 0.7)
    pid = [e for e in eng.entries if e.softcore is not None][0].softcore['pid']
    lam = np.linspace(0.0, 1.0, 21)
    walked = engine_walked = 0
    for _ in range(4):
        integrator.step(3)
        before = eng.ctx.pair_stats(pid)['n_candidate_walks']
        cand = states(eng.ctx, pid, eng.x, lam)
        walked += eng.ctx.pair_stats(pid)['n_candidate_walks'] - before
        before = eng.ctx.pair_stats(pid)['n_candidate_walks']
        via_engine = eng.energies_at_states(['lambda_vdw'], lam[:, None])
        engine_walked += eng.ctx.pair_stats(pid)['n_candidate_walks'] - before
        eng.ctx.set_option('group_candidates', 0)
        full = states(eng.ctx, pid, eng.x, lam)
        eng.ctx.set_option('group_candidates', 1)
        assert np.abs(cand - full).max() <= 1e-12 * np.abs(full).max()
        ref = reference_loop(context, ['lambda_vdw'], lam[:, None])
        assert np.abs(via_engine - ref).max() <= 1e-9 * np.abs(ref).max()
    assert eng.ctx.pair_stats(pid)['n_candidates'] > 30 and walked >= 2 and engine_walked >= 2, (eng.ctx.pair_stats(pid), walked,
                                                                                                 engine_walked)
    for k in (0, 7, 20):
        eng.ctx.pair_set_lambda(pid, lam[k])
        assert cand[k] == pytest.approx(energy_now(eng.ctx, pid, eng.x, eng.n), rel=1e-11, abs=1e-12)
    eng.ctx.pair_set_lambda(pid, 0.7)
