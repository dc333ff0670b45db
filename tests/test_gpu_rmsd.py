"""GPU tests of the RMSD force (csrc/rmsd.hip): the deviation of selected particles from a reference after the best rigid fit, as an
energy and its gradient, on the single-block path and on the three-launch path.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|, against the 50-digit checker of
tests/rmsd_cases.py.  Every case is evaluated once per path and the result shared by the tests that read it; every test prints its
own deviation.  DESIGN.md 3.RM has the worst ones measured on an MI355X."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import rmsd_cases as RC  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402

E_REL, F_REL = 1e-10, 1e-9
BOX = np.full(3, 12.0)


# ------------------------------------------------------------------------------------ the cases
def _noisy(n, seed, noise=0.05):
    ref = RC.blob(n, seed)
    return ref, RC.displaced(ref, seed, noise), None


def _subset():
    ref = RC.blob(300, 31)
    pos = RC.displaced(ref, 32, 0.05)
    sel = np.random.default_rng(33).permutation(300)[:65]
    return ref, pos, [int(p) for p in sel]


def _rigid():
    ref = RC.blob(257, 3)
    return ref, RC.rigid_image(ref, 4), None


def _small_far():
    ref = RC.blob(257, 8, offset=(8.0, 8.0, 8.0))
    return ref, RC.displaced(ref, 9, 1e-3), None


CASES = {
    'n1': lambda: _noisy(1, 11), 'n2': lambda: _noisy(2, 12), 'n3': lambda: _noisy(3, 0),
    'n64': lambda: _noisy(64, 74), 'n65': lambda: _noisy(65, 75), 'n257': lambda: _noisy(257, 267), 'n1025': lambda: _noisy(1025, 1035),
    'subset': _subset, 'rigid': _rigid, 'small_far': _small_far,
    'mirror': lambda: RC.mirror_case(65, 5) + (None,), 'line': lambda: RC.line_case(65, 21) + (None,),
}
BOTH_PATHS = ['n1', 'n2', 'n3', 'n64', 'n65', 'n257', 'n1025', 'subset', 'rigid', 'small_far']
GENERIC = ['n64', 'n65', 'n257', 'n1025']              # well-conditioned: the gap and the deviation are asserted on the checker
RUNS = [(case, blocks) for case in BOTH_PATHS for blocks in (1, 3)] + [('mirror', 0), ('line', 0)]


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(reference, positions, selection or None, the checker's answer): computed once, never changed."""
    ref, pos, sel = CASES[name]()
    ref.setflags(write=False)
    pos.setflags(write=False)
    out = RC.evaluate(pos, ref, sel)
    out['forces'].setflags(write=False)
    return ref, pos, sel, out


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')            # (a copy: the cases are read-only)


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.full((len(pos), 3), np.nan) if start is None else start)       # (every row has to be written)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def make(ctx, ref, sel):
    particles = list(range(len(ref))) if sel is None else sel
    return ctx.rmsd_create(particles, ref[particles])


@functools.lru_cache(maxsize=None)
def run_of(name, blocks):
    """One context per (case, path): two evaluations with the energy, one without, one that accumulates onto a given start."""
    ref, pos, sel, _ = case_of(name)
    ctx = B.HipContext(len(pos), None)
    try:
        ctx.set_option('rmsd_blocks', blocks)
        fid = make(ctx, ref, sel)
        stats = ctx.rmsd_stats(fid)
        e1, f1 = evaluate(ctx, fid, pos)
        e2, f2 = evaluate(ctx, fid, pos)
        _, f3 = evaluate(ctx, fid, pos, energy=False)
        start = np.random.default_rng(99).normal(size=pos.shape)
        _, f4 = evaluate(ctx, fid, pos, accumulate=True, start=start, energy=False)
        ctx.check()
    finally:
        ctx.close()
    return dict(e=e1, f=f1, again=(e2, f2), no_energy=f3, start=start, accumulated=f4, stats=stats)


def assert_close(e, f, out, what):
    e_ref, f_ref = out['energy'], out['forces']
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (checker %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g; gap %.3g, rmsd / rg = %.3g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale,
           out['gap'], e_ref / max(out['rg'], 1e-300)))
    assert np.isfinite(e) and np.isfinite(f).all()
    assert abs(e - e_ref) <= E_REL * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


# ------------------------------------------------------------------------------------ 1. the kernels against the checker
@pytest.mark.parametrize('name,blocks', RUNS)
def test_energy_and_forces_against_the_checker(name, blocks):
    ref, pos, sel, out = case_of(name)
    got = run_of(name, blocks)
    n_sel = len(pos) if sel is None else len(sel)
    assert got['stats']['particles'] == n_sel
    if blocks:                                     # the path that was asked for is the path that ran
        assert got['stats']['blocks'] == blocks and got['stats']['launches_per_eval'] == (1 if blocks == 1 else 3)
    assert_close(got['e'], got['f'], out, '%s, rmsd_blocks = %d' % (name, blocks))
    if name in GENERIC:
        assert out['gap'] >= 0.05 and out['energy'] >= 0.01 * out['rg']
    if name == 'n2':
        assert out['gap'] < 1e-12 and out['energy'] > 0.0            # a degenerate top eigenvalue: the result is unique all the same
    if name == 'n3':
        assert out['gap'] < 0.05 and out['energy'] > 0.0
    if name == 'line':
        assert out['gap'] < 1e-12 and out['energy'] > 0.01           # the rotation about the line is free
    if name == 'mirror':
        assert out['energy'] > 0.5                                   # an improper fit would leave the 0.02 nm of noise
    if name in ('n1', 'rigid'):                                      # the defined zero: exactly, and finite
        assert out['energy'] == 0.0 and got['e'] == 0.0 and not got['f'].any()


@pytest.mark.parametrize('name,blocks', RUNS)
def test_same_positions_same_bits(name, blocks):
    got = run_of(name, blocks)
    e2, f2 = got['again']
    assert e2 == got['e'] and np.array_equal(f2, got['f'])
    assert np.array_equal(got['no_energy'], got['f'])


@pytest.mark.parametrize('name,blocks', RUNS)
def test_forces_and_torques_sum_to_zero(name, blocks):
    _, pos, _, out = case_of(name)
    f = run_of(name, blocks)['f']
    top = np.abs(out['forces']).max()
    total = np.abs(f.sum(axis=0)).max()
    torque = np.abs(np.cross(pos - pos.mean(axis=0), f).sum(axis=0)).max()
    print('%s, rmsd_blocks = %d: |sum F| = %.2e, |sum (x - c) x F| = %.2e of max|F| = %.4g' % (name, blocks, total / max(top, 1e-300),
                                                                                            torque / max(top, 1e-300), top))
    assert total <= 1e-9 * top and torque <= 1e-9 * top


@pytest.mark.parametrize('name,blocks', RUNS)
def test_accumulate_adds_to_what_was_there(name, blocks):
    _, pos, sel, _ = case_of(name)
    got = run_of(name, blocks)
    inside = np.zeros(len(pos), dtype=bool)
    inside[list(range(len(pos))) if sel is None else sel] = True
    # without accumulate the rows outside the selection are exactly zero (the buffer held NaN before) ...
    assert not got['f'][~inside].any() and np.isfinite(got['f']).all()
    # ... with it they keep their contents bit for bit, and a selected row is what it held plus the force: one fp64 addition
    assert np.array_equal(got['accumulated'][~inside], got['start'][~inside])
    assert np.array_equal(got['accumulated'][inside], (got['start'] + got['f'])[inside])
    if name == 'subset':
        assert inside.sum() == 65 and (~inside).sum() == 235


def test_the_library_chooses_the_path_by_the_size_of_the_selection():
    ctx = B.HipContext(6000, None)
    try:
        ref = RC.blob(6000, 41)
        small = ctx.rmsd_create(list(range(64)), ref[:64])
        large = ctx.rmsd_create(list(range(6000)), ref)
        assert ctx.rmsd_stats(small)['blocks'] == 1
        assert ctx.rmsd_stats(large)['blocks'] >= 2 and ctx.rmsd_stats(large)['launches_per_eval'] == 3
        # the two paths agree on a selection neither test above reaches: 6000 particles, 6 blocks against 1
        pos = RC.displaced(ref, 42, 0.05)
        e_many, f_many = evaluate(ctx, large, pos)
        ctx.set_option('rmsd_blocks', 1)
        single = ctx.rmsd_create(list(range(6000)), ref)
        e_one, f_one = evaluate(ctx, single, pos)
        top = np.abs(f_one).max()
        print('6000 particles: %d blocks against 1: dE rel %.2e, dF %.2e of max|F|' % (ctx.rmsd_stats(large)['blocks'], abs(e_many - e_one) / e_one,
                                                                                      np.abs(f_many - f_one).max() / top))
        # both are within the bars of the exact answer, hence within twice the bars of each other
        assert abs(e_many - e_one) <= 2 * E_REL * e_one and np.abs(f_many - f_one).max() <= 2 * F_REL * top
        ctx.check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ 2. through the Python API
def bare_system(n, box=None, mass=12.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(float(mass))
    if box is not None:
        system.setDefaultPeriodicBoxVectors((float(box[0]), 0, 0), (0, float(box[1]), 0), (0, 0, float(box[2])))
    return system


def context_with(system, positions, integrator=None, properties=None):
    context = openmm.Context(system, integrator or openmm.VerletIntegrator(0.001), None, properties)
    context.setPositions(np.asarray(positions) * unit.nanometers)
    return context


def energy_forces(context, **kw):
    state = context.getState(getEnergy=True, getForces=True, **kw)
    return state.getPotentialEnergy()._value, state.getForces(asNumpy=True)._value


def positions_of(context):
    return context.getState(getPositions=True).getPositions(asNumpy=True)._value


def chain_bonds(n, group=0):
    """Harmonic bonds between consecutive particles at the length they have: a second force next to the restraint."""
    bonds = openmm.HarmonicBondForce()
    for i in range(n - 1):
        bonds.addBond(i, i + 1, 0.5, 100.0)
    bonds.setForceGroup(group)
    return bonds


def restraint(reference, particles, k, group=0):
    cv = openmm.CustomCVForce('0.5*k*rmsd^2')
    cv.addGlobalParameter('k', k)
    cv.addCollectiveVariable('rmsd', openmm.RMSDForce(reference, particles))
    cv.setForceGroup(group)
    return cv


@pytest.mark.parametrize('box', [None, BOX], ids=['free space', 'box'])
def test_alone_in_a_force_group(box):
    """40 particles, 17 of them selected in shuffled order, next to harmonic bonds in another group: getState(groups=...) gives the
    checker's energy and forces; a new reference gives the checker's new value.  The positions lie outside the box's first image
    on purpose: they are read raw."""
    n = 40
    ref = RC.blob(n, 51)
    pos = RC.displaced(ref, 52, 0.05)
    sel = [int(p) for p in np.random.default_rng(53).permutation(n)[:17]]
    force = openmm.RMSDForce(ref * unit.nanometers, sel)
    force.setForceGroup(4)
    system = bare_system(n, box)
    system.addForce(chain_bonds(n))
    system.addForce(force)
    context = context_with(system, pos)
    out = RC.evaluate(pos, ref, sel)
    e, f = energy_forces(context, groups={4})
    assert_close(e, f, out, 'RMSDForce alone in group 4 (%s)' % ('box' if box is not None else 'free space'))
    e_all, _ = energy_forces(context)
    e_bonds, _ = energy_forces(context, groups={0})
    assert e_bonds > 0.0 and abs(e_all - (e_bonds + e)) <= 1e-12 * abs(e_all)
    fresh = RC.blob(n, 54)
    force.setReferencePositions(fresh)
    force.updateParametersInContext(context)
    e, f = energy_forces(context, groups={4})
    assert_close(e, f, RC.evaluate(pos, fresh, sel), '... after setReferencePositions + updateParametersInContext')
    assert abs(e - out['energy']) > 0.1
    force.setParticles(sel[:9])                                         # (the number of particles may change)
    force.updateParametersInContext(context)
    e, f = energy_forces(context, groups={4})
    assert_close(e, f, RC.evaluate(pos, fresh, sel[:9]), '... after setParticles: 9 of them')
    context._engine.ctx.check()


@pytest.mark.parametrize('box', [None, BOX], ids=['free space', 'box'])
def test_inside_a_custom_cv_force(box):
    n, k = 40, 250.0
    ref = RC.blob(n, 61)
    pos = RC.displaced(ref, 62, 0.05)
    sel = list(range(5, 30))
    cv = restraint(ref, sel, k)
    system = bare_system(n, box)
    system.addForce(cv)
    context = context_with(system, pos)
    out = RC.evaluate(pos, ref, sel)
    rmsd = out['energy']
    e, f = energy_forces(context)
    (value,) = cv.getCollectiveVariableValues(context)
    outer = dict(energy=0.5 * k * rmsd * rmsd, forces=k * rmsd * out['forces'], gap=out['gap'], rg=out['rg'])
    assert_close(e, f, outer, 'CustomCVForce(0.5*k*rmsd^2) over an RMSDForce (%s)' % ('box' if box is not None else 'free space'))
    print('getCollectiveVariableValues: %.15g (checker %.15g)' % (value, rmsd))
    assert abs(value - rmsd) <= E_REL * rmsd
    context._engine.ctx.check()


def test_minimisation_brings_the_deviation_down():
    n, k = 32, 1.0e4
    ref = RC.blob(n, 71)
    pos = RC.displaced(ref, 72, 0.05)
    cv = restraint(ref, [], k)
    system = bare_system(n)
    system.addForce(cv)
    sim = app.Simulation(app.Topology(n), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(pos * unit.nanometers)
    (before,) = cv.getCollectiveVariableValues(sim.context)
    sim.minimizeEnergy(tolerance=0.01)
    (after,) = cv.getCollectiveVariableValues(sim.context)
    print('minimisation of 0.5*k*rmsd^2 alone: rmsd %.4f -> %.3e nm' % (before, after))
    assert 0.08 < before < 0.1 and after < 1e-3 and math.isfinite(after)
    sim.context._engine.ctx.check()


def thermal(n, mass, seed=5, kT=2.494339):
    return np.random.default_rng(seed).normal(size=(n, 3)) * math.sqrt(kT / mass)


def test_twenty_verlet_steps_with_the_restraint_in_a_group_of_its_own():
    n = 40
    ref = RC.blob(n, 81)
    pos = RC.displaced(ref, 82, 0.05)
    system = bare_system(n, BOX)
    system.addForce(chain_bonds(n, group=0))
    system.addForce(restraint(ref, list(range(0, n, 2)), 500.0, group=7))
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(system, pos, integrator)
    context.setVelocities(thermal(n, 12.0))
    integrator.step(20)
    x = positions_of(context)
    e7, f7 = energy_forces(context, groups={7})
    out = RC.evaluate(x, ref, list(range(0, n, 2)))
    moved = np.abs(x - pos).max()
    print('20 Verlet steps: atoms moved up to %.3e nm; restraint energy %.6g (checker %.6g)' % (moved, e7, 250.0 * out['energy'] ** 2))
    assert np.isfinite(x).all() and moved > 1e-3
    assert abs(e7 - 250.0 * out['energy'] ** 2) <= E_REL * e7
    context._engine.ctx.check()


def test_twenty_respa_steps_with_the_restraint_in_the_outer_group():
    """RESPA [2, 1]: the bonds in the inner group 0, the restraint alone in group 1 -- the group leaves the fused inner loop."""
    n = 40
    ref = RC.blob(n, 81)
    pos = RC.displaced(ref, 82, 0.05)
    system = bare_system(n, BOX)
    system.addForce(chain_bonds(n, group=0))
    system.addForce(restraint(ref, list(range(0, n, 2)), 500.0, group=1))
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = context_with(system, pos, integrator)
    context.setVelocities(thermal(n, 12.0))
    integrator.step(20)
    x = positions_of(context)
    moved = np.abs(x - pos).max()
    print('20 RESPA [2, 1] steps: atoms moved up to %.3e nm' % moved)
    assert np.isfinite(x).all() and moved > 1e-3
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 3. refusals at the C-ABI
def test_abi_refusals_name_the_family():
    n = 8
    ref = RC.blob(n, 91)
    ctx = B.HipContext(n, BOX)
    try:
        for particles, rows in (([0, 3, 3], ref[[0, 3, 3]]), ([0, 8], ref[[0, 1]]), ([-1, 2], ref[[0, 2]]), ([], ref[:0])):
            with pytest.raises(B.HipError, match='amm_rmsd_create: .*AMM_FORCE_RMSD'):
                ctx.rmsd_create(particles, rows)
        fid = ctx.rmsd_create([1, 2, 5], ref[[1, 2, 5]])
        pos = RC.displaced(ref, 92, 0.05)
        before = evaluate(ctx, fid, pos)
        # a refused change leaves the force as it was
        with pytest.raises(B.HipError, match='amm_rmsd_set_reference: .*listed twice.*AMM_FORCE_RMSD'):
            ctx.rmsd_set_reference(fid, [1, 1], ref[[1, 1]])
        after = evaluate(ctx, fid, pos)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        # an id of another family
        prog = X.compile_term('x*x', ('x', 'y', 'z'), [], [])
        rows = np.full((n, 4), -1, dtype=np.int32)
        rows[:, 0] = np.arange(n)
        other = ctx.term_expr_create(B.TERM_EXTERNAL, prog.code, prog.consts, [], rows, np.zeros((0, 1)))
        with pytest.raises(B.HipError) as err:
            ctx.rmsd_set_reference(other, [0, 1], ref[[0, 1]])
        assert str(err.value) == ('amm_rmsd_set_reference: not the id of an RMSD force (AMM_FORCE_RMSD): force %d is a term-expression force '
                                  '(AMM_FORCE_TERM_EXPR: amm_term_expr_*)' % other)
        with pytest.raises(B.HipError, match=r'amm_term_expr_release: not a term-expression force id: force %d is an RMSD force '
                                             r'\(AMM_FORCE_RMSD: amm_rmsd_\*\)' % fid):
            ctx.term_expr_release(fid)
        # several ranks
        with pytest.raises(B.HipError) as err:
            B._chk(B.lib().amm_set_slice(ctx.h, 0, 2))
        assert str(err.value) == 'amm_set_slice: an RMSD force (AMM_FORCE_RMSD) runs on a single rank'
        # released: its own entry points refuse it bare, the evaluation as a released id
        ctx.rmsd_release(fid)
        with pytest.raises(B.HipError) as err:
            ctx.rmsd_release(fid)
        assert str(err.value) == 'amm_rmsd_release: not the id of an RMSD force (AMM_FORCE_RMSD)'
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, pos)
        B._chk(B.lib().amm_set_slice(ctx.h, 0, 2))                    # nothing single-rank is left
        B._chk(B.lib().amm_set_slice(ctx.h, 0, 1))
        with pytest.raises(B.HipError, match='amm_set_option: rmsd_blocks'):
            ctx.set_option('rmsd_blocks', 1025)
        ctx.check()
    finally:
        ctx.close()
