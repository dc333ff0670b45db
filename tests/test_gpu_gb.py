"""GPU tests of the generalized-Born force (GBSAOBCForce; csrc/gb.hip) against the fp64 restatement of its definition in torch on the
CPU (tests/gb_cases.py, forces by autograd), through the C-ABI and through the AtomsMM-shaped API.

Tolerances are the project's own: energies rel 1e-10, forces 1e-9 max|F|; Born radii rel 1e-12.  Inputs: n = 1
and n = 2; N5, five atoms that take every branch of the Born integrand; S33, the 33-atom solute of
hydroxyethylaminoanthraquinone-in-water; D1527, the first 509 waters of q-SPC-FW (six j tiles, not a multiple of 64 or 256); D4608,
that box three times in a row (18 tiles, 16 lanes per row).  Every one with NoCutoff and with a 1.0 nm cutoff.

Worst deviations measured on an MI355X (every test prints its own): energy rel 4.6e-15, forces 7.6e-15 of max|F|, Born
radii rel 2.9e-15; RESPA against the CPU loop max|dx| 0, max|dv| 4.0e-15 nm/ps; Verlet drift 0.82 kJ/mol without the GB force, 0.19 with."""
import io
import os

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
from oracle import oracle as O  # noqa: E402  (checker only)
from conftest import GOLDEN  # noqa: E402
from free_space_cases import descriptors, oracle_bonded, oracle_pair  # noqa: E402
import gb_cases as G  # noqa: E402

E_REL, F_REL, B_REL = 1e-10, 1e-9, 1e-12
NOCUTOFF = descriptors()['nocutoff'][1]


@pytest.fixture(scope='module')
def cases(heaq, spcfw):
    return {'n1': G.tiny(1), 'n2': G.tiny(2), 'N5': G.n5(), 'S33': G.with_radii(G.s33(heaq)), 'D1527': G.with_radii(G.d1527(spcfw)),
            'D4608': G.d4608(spcfw)}


@pytest.fixture(scope='module')
def references(cases):
    """The restatement per (case, cutoff), computed once and never written to."""
    table = {}

    def get(case, rc):
        if (case, rc) not in table:
            out = G.evaluate(cases[case], rc)
            for key in ('forces', 'born'):
                out[key].setflags(write=False)
            table[(case, rc)] = out
        return table[(case, rc)]
    return get


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def create(ctx, c, rc=None, **kw):
    return ctx.gb_create(c['charge'], c['radius'], c['scale'], rc=rc or 0.0, **kw)


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, pos, f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def assert_close(e, f, ref, what):
    scale = np.abs(ref['forces']).max()
    print('%s: E = %.15g (restatement %.15g, rel %.2e)  max|dF| = %.3e of max|F| = %.6g' %
          (what, e, ref['energy'], abs(e - ref['energy']) / abs(ref['energy']), np.abs(f - ref['forces']).max(), scale))
    assert e == pytest.approx(ref['energy'], rel=E_REL)
    if scale == 0.0:
        assert not f.any()                       # one atom: zeros, not small numbers
    else:
        assert np.abs(f - ref['forces']).max() <= F_REL * scale


# ------------------------------------------------------------------------------------ 1. the C-ABI against the restatement
@pytest.mark.parametrize('rc', [None, 1.0])
@pytest.mark.parametrize('case', ['n1', 'n2', 'N5', 'S33', 'D1527', 'D4608'])
def test_abi_parity(cases, references, case, rc):
    c = cases[case]
    n = len(c['positions'])
    ref = references(case, rc)
    ctx = B.HipContext(n, None)                  # no periodic box at all
    try:
        fid = create(ctx, c, rc)
        pos = dev(c['positions'])
        born = ctx.gb_born_radii(fid, pos)
        print('%s rc %s: max rel Born radius error %.2e' % (case, rc, np.abs(born / ref['born'] - 1).max()))
        assert np.abs(born / ref['born'] - 1).max() <= B_REL
        e, f = evaluate(ctx, fid, pos)
        assert_close(e, f, ref, '%s / rc %s' % (case, rc))
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
        assert np.array_equal(ctx.gb_born_radii(fid, pos), born)
        ctx.check()
    finally:
        ctx.close()


def test_a_gb_force_in_a_context_with_a_box_ignores_the_box(cases, references):
    c = cases['S33']
    ctx = B.HipContext(33, np.full(3, 1.5))      # smaller than the solute's reach: a minimum image would change the sums
    try:
        e, f = evaluate(ctx, create(ctx, c), dev(c['positions']))
        assert_close(e, f, references('S33', None), 'S33 in a context with a box')
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 2. lanes per row
@pytest.mark.parametrize('width', [1, 2, 4, 8, 16, 32, 64])
def test_every_lane_width(cases, references, width):
    c = cases['D1527']
    ctx = B.HipContext(len(c['positions']), None)
    try:
        ctx.set_option('gb_lanes_per_row', width)
        fid = create(ctx, c, 1.0)
        pos = dev(c['positions'])
        assert np.abs(ctx.gb_born_radii(fid, pos) / references('D1527', 1.0)['born'] - 1).max() <= B_REL
        e, f = evaluate(ctx, fid, pos)
        assert_close(e, f, references('D1527', 1.0), 'D1527 / %d lanes per row' % width)
        ctx.check()
    finally:
        ctx.close()


@pytest.mark.parametrize('case,auto,other', [('D1527', 64, 32), ('D4608', 16, 32)])
def test_the_automatic_width(cases, case, auto, other):
    """The order of summation, hence the bits, is the width's: the automatic choice gives the bits of the width it should be (64 up to
    2048 atoms, 16 at 4608) and not those of another."""
    c = cases[case]
    pos = dev(c['positions'])
    rows = {}
    for width in (0, auto, other):
        ctx = B.HipContext(len(c['positions']), None)
        try:
            ctx.set_option('gb_lanes_per_row', width)
            rows[width] = evaluate(ctx, create(ctx, c), pos)
            ctx.check()
        finally:
            ctx.close()
    assert rows[0][0] == rows[auto][0] and np.array_equal(rows[0][1], rows[auto][1])
    assert not np.array_equal(rows[0][1], rows[other][1])


def test_the_width_option_is_checked():
    ctx = B.HipContext(4, None)
    try:
        for bad in (3, 128, -1):
            with pytest.raises(B.HipError, match='gb_lanes_per_row is 0 .automatic. or a power of two up to 64'):
                ctx.set_option('gb_lanes_per_row', bad)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 3. new parameters, same positions
def test_set_params_at_the_same_positions(cases, references):
    c = cases['S33']
    ctx = B.HipContext(33, None)
    try:
        fid = create(ctx, c)
        pos = dev(c['positions'])
        e0, _ = evaluate(ctx, fid, pos)
        scaled = 0.5 * c['charge']
        ctx.gb_set_params(fid, scaled, c['radius'], c['scale'], eps_in=2.0, eps_out=40.0, sa_energy=3.0, rc=0.0)
        ref = G.evaluate(c, None, eps_in=2.0, eps_out=40.0, sa=3.0, charge=scaled)
        assert abs(ref['energy'] - e0) > 1.0
        e1, f1 = evaluate(ctx, fid, pos)
        assert_close(e1, f1, ref, 'S33 / half charges, dielectrics 2 and 40, surface energy 3')
        # a cutoff where there was none, and new radii: the Born radii follow
        radius = c['radius'] * 1.1
        ctx.gb_set_params(fid, c['charge'], radius, c['scale'], rc=1.0)
        ref = G.evaluate(dict(c, radius=radius), 1.0)
        assert np.abs(ctx.gb_born_radii(fid, pos) / ref['born'] - 1).max() <= B_REL
        e2, f2 = evaluate(ctx, fid, pos)
        assert_close(e2, f2, ref, 'S33 / radii x 1.1, rc 1.0')
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 4. the API, static
def add_gb(system, c, group, method=None, cutoff=1.0):
    gb = openmm.GBSAOBCForce()
    for q, r, s in zip(c['charge'], c['radius'], c['scale']):
        gb.addParticle(float(q), float(r), float(s))
    if method is not None:
        gb.setNonbondedMethod(method)
    gb.setCutoffDistance(cutoff)
    gb.setForceGroup(group)
    system.addForce(gb)
    return gb


GROUPS = {openmm.HarmonicBondForce: 0, openmm.HarmonicAngleForce: 1, openmm.PeriodicTorsionForce: 2, openmm.NonbondedForce: 3,
          openmm.GBSAOBCForce: 4}


def check_static(context, raw, positions, gb_ref):
    """Every group and the total against the oracle (bonded terms, exceptions, pair force) and the restatement (group 4)."""
    raw = dict(raw, positions=positions)
    bonded = oracle_bonded(raw)
    e_pair, f_pair, _ = oracle_pair(NOCUTOFF, raw)
    want = {0: bonded['bonds'], 1: bonded['angles'], 2: bonded['torsions'],
            3: (e_pair + bonded['exceptions'][0], f_pair + bonded['exceptions'][1]), 4: (gb_ref['energy'], gb_ref['forces'])}
    for group, (e_ref, f_ref) in want.items():
        state = context.getState(getEnergy=True, getForces=True, groups={group})
        e, f = state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value
        print('group %d: E = %.15g (reference %.15g)  max|dF| = %.3e of %.6g' % (group, e, e_ref, np.abs(f - f_ref).max(), np.abs(f_ref).max()))
        assert e == pytest.approx(e_ref, rel=E_REL)
        assert np.abs(f - f_ref).max() <= F_REL * np.abs(f_ref).max()
    total_f = sum(f for _, f in want.values())
    state = context.getState(getEnergy=True, getForces=True)
    assert state.getPeriodicBoxVectors() is None
    assert state.getPotentialEnergy()._value == pytest.approx(sum(e for e, _ in want.values()), rel=E_REL)
    assert np.abs(state.getForces(asNumpy=True)._value - total_f).max() <= F_REL * np.abs(total_f).max()
    context._engine.ctx.check()


def test_api_static_s33(cases, references, heaq):
    raw = G.s33(heaq)
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    add_gb(system, cases['S33'], 4)
    for force in system.getForces():
        force.setForceGroup(GROUPS[type(force)])
    context = openmm.Context(system, openmm.VerletIntegrator(0.0))
    assert context._engine.free_space
    context.setPositions(raw['positions'] * unit.nanometers)
    check_static(context, raw, raw['positions'], references('S33', None))
    # updateParametersInContext through the API: the new reference, not the old one
    (gb,) = [f for f in system.getForces() if isinstance(f, openmm.GBSAOBCForce)]
    gb.setSolventDielectric(20.0)
    for k in range(33):
        q, r, s = gb.getParticleParameters(k)
        gb.setParticleParameters(k, 0.8 * q, r, s)
    gb.updateParametersInContext(context)
    check_static(context, raw, raw['positions'], G.evaluate(cases['S33'], None, eps_out=20.0, charge=0.8 * cases['S33']['charge']))


def test_api_static_forcefield_route(cases, heaq):
    """PDB text without CRYST1 -> ForceField(the fixture's file, the <GBSAOBCForce> section) -> createSystem -> a Context."""
    with open(os.path.join(GOLDEN, 'data', 'hydroxyethylaminoanthraquinone-in-water.pdb')) as fh:
        lines = [line for line in fh if line[:6] != 'CRYST1']
    atoms = [line for line in lines if line[:6] in ('ATOM  ', 'HETATM')][:33]
    pdb = app.PDBFile(io.StringIO(''.join(atoms + [line for line in lines if line[:6] == 'CONECT'] + ['END\n'])))
    forcefield = app.ForceField(os.path.join(GOLDEN, 'data', 'hydroxyethylaminoanthraquinone-in-water.xml'),
                                os.path.join(GOLDEN, 'data', 'gbsa-obc-heaq.xml'))
    system = forcefield.createSystem(pdb.topology, rigidWater=False, removeCMMotion=False, solventDielectric=60.0)
    for force in system.getForces():
        force.setForceGroup(GROUPS[type(force)])
    positions = np.array([[v[0], v[1], v[2]] for v in pdb.positions._value], dtype=np.float64)
    d = forcefield.describe(pdb.topology)
    raw = {key: d[key] for key in ('charge', 'sigma', 'epsilon', 'mass', 'bonds', 'bond_r0', 'bond_k', 'angles', 'angle_theta0', 'angle_k',
                                   'torsions', 'torsion_n', 'torsion_phase', 'torsion_k', 'exc_pairs', 'exc_chargeprod', 'exc_sigma',
                                   'exc_epsilon')}
    context = openmm.Context(system, openmm.VerletIntegrator(0.0))
    context.setPositions(pdb.positions)
    c = dict(cases['S33'], positions=positions, charge=d['charge'])
    check_static(context, raw, positions, G.evaluate(c, None, eps_out=60.0))


# ------------------------------------------------------------------------------------ 5. the API, dynamics
def test_verlet_energy_drift_with_and_without_gb(cases, heaq):
    """200 steps of VerletIntegrator(0.5 fs) on the solute: the total-energy drift with the GB force is at most twice the drift of the
    same run without it (GB adds a smooth force of comparable size)."""
    raw = G.s33(heaq)
    drift = {}
    for with_gb in (False, True):
        system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
        if with_gb:
            add_gb(system, cases['S33'], 1)
        integrator = openmm.VerletIntegrator(0.5 * unit.femtoseconds)
        context = openmm.Context(system, integrator)
        context.setPositions(raw['positions'] * unit.nanometers)
        context.setVelocitiesToTemperature(300 * unit.kelvin, 4)

        def total():
            s = context.getState(getEnergy=True)
            return s.getPotentialEnergy()._value + s.getKineticEnergy()._value
        e0 = total()
        integrator.step(200)
        drift[with_gb] = abs(total() - e0)
        context._engine.ctx.check()
    print('Verlet 200 x 0.5 fs on S33: |dE| = %.6g kJ/mol without GB, %.6g kJ/mol with GB' % (drift[False], drift[True]))
    assert drift[True] <= 2.0 * drift[False]


def test_respa_dynamics_vs_cpu_loop(cases, heaq):
    """RespaPropagator([2, 1]) at 1 fs, 3 steps: bonded terms, exceptions and the pair force in group 0, the GB force in group 1 (the
    outer one), against the same velocity-Verlet / RESPA loop on the CPU over oracle + restatement forces.  Bounds: those of
    test_gpu_free_space.py::test_respa_dynamics_vs_oracle."""
    raw = G.s33(heaq)
    c = cases['S33']
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    add_gb(system, c, 1)
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    simulation = app.Simulation(app.Topology(33), system, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(raw['positions'] * unit.nanometers)
    simulation.context.setVelocitiesToTemperature(300 * unit.kelvin, 1)
    v0 = simulation.context.getState(getVelocities=True).getVelocities(asNumpy=True)._value.copy()
    nsteps = 3
    simulation.step(nsteps)
    state = simulation.context.getState(getPositions=True, getVelocities=True, getEnergy=True)
    dt, m = 0.001, raw['mass']

    def inner(p, wf=True):
        at = dict(raw, positions=p)
        e_pair, f_pair, _ = oracle_pair(NOCUTOFF, at)
        parts = list(oracle_bonded(raw, p, want_forces=wf).values())
        return e_pair + sum(e for e, _ in parts), (f_pair + sum(f for _, f in parts)) if wf else None

    def outer(p, wf=True):
        out = G.evaluate(dict(c, positions=p), None, want_forces=wf)
        return out['energy'], out.get('forces')
    x, v = raw['positions'].copy(), v0.copy()
    F0 = inner(x)[1]
    for _ in range(nsteps):
        F1 = outer(x)[1]
        O.kick(v, F1, m, 0.5 * dt)
        for _n0 in range(2):
            O.kick(v, F0, m, 0.25 * dt)
            O.move(x, v, 0.5 * dt)
            F0 = inner(x)[1]
            O.kick(v, F0, m, 0.25 * dt)
        F1 = outer(x)[1]
        O.kick(v, F1, m, 0.5 * dt)
    dx = np.abs(state.getPositions(asNumpy=True)._value - x).max()
    dv = np.abs(state.getVelocities(asNumpy=True)._value - v).max()
    e_ref = inner(x, False)[0] + outer(x, False)[0]
    print('RESPA with GB outside: max|dx| = %.3e nm, max|dv| = %.3e nm/ps, E = %.15g (reference %.15g)' %
          (dx, dv, state.getPotentialEnergy()._value, e_ref))
    assert dx < 1e-11
    assert dv < 1e-9
    assert state.getPotentialEnergy()._value == pytest.approx(e_ref, rel=1e-10)
    simulation.context._engine.ctx.check()


def test_minimize_energy_with_gb(cases, heaq):
    raw = G.s33(heaq)
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    add_gb(system, cases['S33'], 1)
    simulation = app.Simulation(app.Topology(33), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(raw['positions'] * unit.nanometers)
    e0 = simulation.context.getState(getEnergy=True).getPotentialEnergy()._value
    info = simulation.context._engine.minimize(10.0, 50, None)
    e1 = simulation.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('minimize S33 + GB: %.6f -> %.6f kJ/mol in %d iterations (%s)' % (e0, e1, info['iterations'], info['reason']))
    assert e1 < e0 and e1 == pytest.approx(info['energy'], rel=1e-9)
    # the minimum found is one of the energy the restatement defines
    x = simulation.context.getState(getPositions=True).getPositions(asNumpy=True)._value
    gb_only = simulation.context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value
    assert gb_only == pytest.approx(G.evaluate(dict(cases['S33'], positions=x), None, want_forces=False)['energy'], rel=E_REL)
    simulation.minimizeEnergy(maxIterations=5)           # the public entry point
    assert simulation.context.getState(getEnergy=True).getPotentialEnergy()._value <= e1 + 1e-9 * abs(e1)
    simulation.context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 6. refusals
def test_the_library_refuses_bad_parameters_and_wrong_ids(cases):
    c = cases['N5']
    ctx = B.HipContext(5, None)
    try:
        with pytest.raises(B.HipError, match='particle 2: radius .* is not above the dielectric offset'):
            ctx.gb_create(c['charge'], np.array([0.3, 0.1, 0.009, 0.12, 0.2]), c['scale'])
        with pytest.raises(B.HipError, match='particle 4: negative scale'):
            ctx.gb_create(c['charge'], c['radius'], np.array([1.0, 0.8, 0.72, 0.85, -0.1]))
        for kw in (dict(eps_in=0.0), dict(eps_out=-1.0)):
            with pytest.raises(B.HipError, match='dielectrics must be positive'):
                create(ctx, c, **kw)
        fid = create(ctx, c)
        with pytest.raises(B.HipError, match='amm_gb_set_params: .*dielectrics must be positive'):
            ctx.gb_set_params(fid, c['charge'], c['radius'], c['scale'], eps_out=0.0)
        bid = ctx.bonded_create()
        pos = dev(c['positions'])
        with pytest.raises(B.HipError, match='not the id of a generalized-Born force'):
            ctx.gb_born_radii(bid, pos)
        with pytest.raises(B.HipError, match='is a generalized-Born force'):
            ctx.pair_set_params(fid, c['charge'], c['charge'], c['charge'])
        e, _ = evaluate(ctx, fid, pos)                        # the refused calls changed nothing
        assert e == pytest.approx(G.evaluate(c)['energy'], rel=E_REL)
        ctx.gb_release(fid)
        with pytest.raises(B.HipError, match='released'):
            evaluate(ctx, fid, pos)
        with pytest.raises(B.HipError, match='not the id of a generalized-Born force'):
            ctx.gb_release(fid)
        ctx.check()
    finally:
        ctx.close()


def test_the_size_limit_is_named():
    n = 32769
    ctx = B.HipContext(n, None)
    try:
        with pytest.raises(B.HipError, match='at most 32768 atoms'):
            ctx.gb_create(np.zeros(n), np.full(n, 0.15), np.full(n, 0.8))          # nothing is evaluated
    finally:
        ctx.close()


def test_the_engine_refuses_on_the_gpu_path_as_on_the_host(cases, heaq, spcfw):
    raw = G.s33(heaq)
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    add_gb(system, cases['S33'], 1, method=openmm.GBSAOBCForce.CutoffPeriodic)
    with pytest.raises(InputError, match='GBSAOBCForce: CutoffPeriodic is not supported'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    water = G.d1527(spcfw)
    system = system_from_arrays(dict(water, box=np.full(3, 4.0)), nonbondedMethod='CutoffPeriodic')
    add_gb(system, cases['D1527'], 1)
    with pytest.raises(InputError, match='a GBSAOBCForce in a System with a box-periodic NonbondedForce'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    with pytest.raises(NotImplementedError, match='the virial of a GBSAOBCForce'):
        atomsmm.PressureComputer(system, app.Topology(1527), openmm.Platform.getPlatformByName('HIP'))
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    add_gb(system, dict(cases['S33'], charge=cases['S33']['charge'][:32]), 1)
    with pytest.raises(openmm.OpenMMException, match='GBSAOBCForce must have exactly as many particles'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    system = system_from_arrays(raw, nonbondedMethod='NoCutoff')
    gb = add_gb(system, cases['S33'], 1)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, lambda\) through a GBSAOBCForce'):
        context._engine.energy_derivative('lambda')
    # a radius the library refuses, at updateParametersInContext: named, and the Context keeps its parameters
    context.setPositions(raw['positions'] * unit.nanometers)
    e0 = context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value
    gb.setParticleParameters(0, 0.1, 0.005, 0.8)
    with pytest.raises(InputError, match='GBSAOBCForce: amm_gb_set_params: particle 0: radius'):
        gb.updateParametersInContext(context)
    assert context.getState(getEnergy=True, groups={1}).getPotentialEnergy()._value == e0
    context._engine.ctx.check()
