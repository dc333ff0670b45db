"""GPU tests of the hydrogen-bond force (csrc/hbond.hip): CustomHbondForce with any energy text over all donor-acceptor pairs -- two
passes over ordered pairs, survivors of the cutoff and the exclusions queued in LDS for the interpreter, forces parked per (row,
chunk) and gathered per atom.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|, 1e-12 nm for the short
trajectories.  References: tests/hbond_cases.py (the text rewritten over p1 .. p6 at 50 digits, forces by mpmath.diff in the atoms' own
coordinates) on the two smallest shapes, and everywhere a CustomCompoundBondForce that holds the surviving pairs -- enumerated on the
host -- as explicit bonds of six particles.

Worst deviations measured on an MI355X (every test prints its own): against the 50-digit reference on 1 x 1 and 1 x 65
pairs, V = 1, 3, 16 -- energy rel 4.1e-16, forces 8.4e-16 of max|F|; against explicit bonds on the six shapes -- 2.0e-16 and 2.9e-15 (V = 16,
64 x 257); 1, 2 and 5 chunks per row -- 1.5e-16 and 9.7e-16; cutoffs at 0, 1.7 / 3.5, 11.9 / 19.2 and 100 % survival -- 1.3e-16 and 1.2e-15;
exclusions -- 1.4e-16 and 7.6e-16; shared atoms -- 1.8e-16 and 3.0e-16; parameters -- 2.1e-16 and 1.9e-16, updates the bits of a fresh Context;
two evaluations, with and without energy -- the same bits; 20 Verlet steps -- 1.1e-15 nm; 4 RESPA steps with fusion on and off -- the same bits;
minimisation -636.6 -> -1680.2 kJ/mol; 50 Langevin-middle steps with the barostat -- the energy of a fresh Context, rel 0."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import hbond_cases as H  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402

E_REL, F_REL, X_ABS = 1e-10, 1e-9, 1e-12
EDGE = 2.5
BOX = np.full(3, EDGE)
METHODS = dict(NoCutoff=0, CutoffNonPeriodic=1, CutoffPeriodic=2)


def assert_close(e, f, e_ref, f_ref, what, e_rel=E_REL):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= e_rel * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


def hbond_force(name, donors, acceptors, dpar, apar, exclusions=(), method='NoCutoff', cutoff=0.9, gvalues=None, group=0, text=None):
    case = H.TEXTS[name]
    force = openmm.CustomHbondForce(text or case['text'])
    for p in case['dnames']:
        force.addPerDonorParameter(p)
    for p in case['anames']:
        force.addPerAcceptorParameter(p)
    for g, value in (case['globals'] if gvalues is None else gvalues).items():
        force.addGlobalParameter(g, value)
    for members, row in zip(donors, dpar):
        force.addDonor(int(members[0]), int(members[1]), int(members[2]), [float(v) for v in row])
    for members, row in zip(acceptors, apar):
        force.addAcceptor(int(members[0]), int(members[1]), int(members[2]), [float(v) for v in row])
    for d, a in exclusions:
        force.addExclusion(int(d), int(a))
    force.setNonbondedMethod(METHODS[method])
    force.setCutoffDistance(cutoff * unit.nanometers)
    force.setForceGroup(group)
    return force


def twin_force(name, donors, acceptors, dpar, apar, pairs, periodic=False, gvalues=None, group=0):
    """The CustomCompoundBondForce that holds `pairs` as explicit bonds of six particles."""
    case = H.compound_case(name, gvalues)
    force = openmm.CustomCompoundBondForce(6, case['text'])
    for p in case['names']:
        force.addPerBondParameter(p)
    for g, value in case['globals'].items():
        force.addGlobalParameter(g, value)
    for d, a in pairs:
        force.addBond(H.members_of(donors, acceptors, (d, a)), [float(v) for v in list(dpar[d]) + list(apar[a])])
    force.setUsesPeriodicBoundaryConditions(periodic)
    force.setForceGroup(group)
    return force


def bare_system(n, box=None, mass=12.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(float(mass))
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


def one_force(n, box, force, positions):
    system = bare_system(n, box)
    system.addForce(force)
    context = context_with(system, positions)
    e, f = energy_forces(context)
    context._engine.ctx.check()
    return e, f, context


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.zeros((len(pos), 3)) if start is None else start)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


def water(n_mol, edge, seed, cutoff):
    """A water-like layout none of whose pairs lies within the margin of the cutoff."""
    pos, donors, acceptors, excl = H.water_layout(n_mol, edge, seed)
    assert H.margin_ok(pos, donors, acceptors, cutoff, np.full(3, edge)) and H.margin_ok(pos, donors, acceptors, cutoff)
    return pos, donors, acceptors, excl


# ------------------------------------------------------------------------------------ 1. fails without the feature
def test_the_class_runs_in_a_context():
    """On the parent commit: AttributeError, openmm has no CustomHbondForce."""
    edge, rc = 1.25, 0.35
    pos, donors, acceptors, excl = water(64, edge, 7, rc)
    force = hbond_force('distance-angle', donors, acceptors, np.zeros((128, 0)), np.zeros((64, 0)), excl, 'CutoffPeriodic', rc)
    e, f, context = one_force(len(pos), np.full(3, edge), force, pos)
    (entry,) = context._engine.entries
    assert entry.term_expr and len(entry.term_ids) == 1 and entry.bonded_id is None
    assert entry.hbond['variables'] == [('distance', (0, 3)), ('angle', (1, 0, 3))]
    expected = H.survivors(pos, donors, acceptors, excl, rc, np.full(3, edge))
    stats = context._engine.hbond_stats(force)
    print('64 molecules, CutoffPeriodic %.2f nm: E = %.12g kJ/mol, max|F| = %.6g, %s (host: %d pairs)' % (rc, e, np.abs(f).max(), stats, len(expected)))
    assert math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1e-3
    assert stats['scanned'] == 128 * 64 and stats['survivors'] == len(expected) > 0 and stats['launches'] >= 3
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()


# ------------------------------------------------------------------------------------ 2. lane, tile and queue boundaries
SHAPES = ((1, 1), (1, 65), (63, 64), (65, 1), (64, 257), (130, 130))
SHAPE_TEXTS = ('distance', 'three', 'sixteen')
REFERENCE_SEEDS = {(1, 1): 3, (1, 65): 11}           # tests/test_hbond_host.py: the filter keeps 95 % with these


def shape_layout(shape):
    return H.layout(shape[0], shape[1], EDGE, REFERENCE_SEEDS.get(shape, 100 + shape[0] + shape[1]))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', SHAPE_TEXTS)
def test_shapes_against_explicit_bonds(name, shape):
    D, A = shape
    pos, donors, acceptors = shape_layout(shape)
    dpar, apar = H.parameters(name, D, 'd', 5), H.parameters(name, A, 'a', 5)
    e, f, context = one_force(len(pos), None, hbond_force(name, donors, acceptors, dpar, apar), pos)
    stats = context._engine.hbond_stats(context._engine.entries[0].force)
    assert len(context._engine.entries[0].hbond['variables']) == H.N_VARIABLES[name]
    assert stats['scanned'] == D * A and stats['survivors'] == D * A
    pairs = H.survivors(pos, donors, acceptors)
    e_ref, f_ref, _ = one_force(len(pos), None, twin_force(name, donors, acceptors, dpar, apar, pairs), pos)
    assert_close(e, f, e_ref, f_ref, '%s (V = %d), %d x %d, %d chunks per donor row, against %d explicit bonds' % (
        name, H.N_VARIABLES[name], D, A, stats['chunks'], len(pairs)))


@pytest.fixture(scope='module')
def shape_references():
    """(layout, parameters, reference) per (text, shape), computed once and never written to."""
    made = {}

    def get(name, shape):
        if (name, shape) not in made:
            pos, donors, acceptors = shape_layout(shape)
            dpar, apar = H.parameters(name, shape[0], 'd', 5), H.parameters(name, shape[1], 'a', 5)
            pairs = H.survivors(pos, donors, acceptors)
            made[name, shape] = (pos, donors, acceptors, dpar, apar, pairs) + H.reference(name, pos, donors, acceptors, dpar, apar, pairs)
        return made[name, shape]
    return get


@pytest.mark.parametrize('shape', SHAPES[:2], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', SHAPE_TEXTS)
def test_smallest_shapes_against_the_50_digit_reference(shape_references, name, shape):
    pos, donors, acceptors, dpar, apar, pairs, e_ref, f_ref, kept, looked = shape_references(name, shape)
    assert looked == shape[0] * shape[1] and len(kept) >= H.MIN_KEPT * looked
    dropped = sorted(set(pairs) - set(kept))         # (the pairs the filter drops are excluded from the force)
    e, f, context = one_force(len(pos), None, hbond_force(name, donors, acceptors, dpar, apar, dropped), pos)
    assert context._engine.hbond_stats(context._engine.entries[0].force)['survivors'] == len(kept)
    assert_close(e, f, e_ref, f_ref, '%s (V = %d), %d x %d against the 50-digit reference over %d of %d pairs' % (
        name, H.N_VARIABLES[name], shape[0], shape[1], len(kept), looked))


@pytest.mark.parametrize('chunks', (1, 2, 5))
def test_chunks_are_summed_in_order(chunks):
    """Option hbond_chunks at the C-ABI: the same pairs in 1, 2 and 5 chunks per row agree with the explicit bonds."""
    D, A = 3, 300
    pos, donors, acceptors = H.layout(D, A, EDGE, 21)
    prog, table = X.compile_hbond(H.TEXTS['three']['text'], [], [], list(H.TEXTS['three']['globals']))
    ctx = B.HipContext(len(pos), None)
    try:
        ctx.set_option('hbond_chunks', chunks)
        fid = ctx.hbond_create(prog.code, prog.consts, [H.TEXTS['three']['globals'][g] for g in prog.globals_],
                               [dict(distance=B.CVAR_DISTANCE, angle=B.CVAR_ANGLE, dihedral=B.CVAR_DIHEDRAL)[k] for k, _ in table],
                               [list(s) for _, s in table], donors, acceptors, np.zeros((0, D)), np.zeros((0, A)))
        e, f = evaluate(ctx, fid, pos)
        stats = ctx.hbond_stats(fid)
        ctx.check()
    finally:
        ctx.close()
    assert stats['chunks'] == chunks and stats['survivors'] == D * A
    e_ref, f_ref, _ = one_force(len(pos), None, twin_force('three', donors, acceptors, np.zeros((D, 0)), np.zeros((A, 0)),
                                                           H.survivors(pos, donors, acceptors)), pos)
    assert_close(e, f, e_ref, f_ref, 'three, 3 x 300 in %d chunks per row' % chunks)


# ------------------------------------------------------------------------------------ 3. cutoffs
@pytest.mark.parametrize('method', ('CutoffNonPeriodic', 'CutoffPeriodic'))
@pytest.mark.parametrize('rate', ('none', 'three-percent', 'twenty-percent', 'all'))
def test_cutoffs_against_explicit_bonds(rate, method):
    """The 2.5 nm box and the 0.9 nm cutoff, 130 donors against 130 acceptors (tests/hbond_cases.py: cutoff_layout): survival near
    0 % (an empty queue), near 3 % (a row keeps about 4 of its 130 columns: the queue drains at the end of a row only), 20 % and 100 %
    (the queue drains in the middle of a row).  Pairs straddle a face, so the minimum image differs from the raw displacement."""
    periodic = method == 'CutoffPeriodic'
    rc = H.CUTOFF
    pos, donors, acceptors = H.cutoff_layout(rate)
    box = BOX if periodic else None
    assert H.margin_ok(pos, donors, acceptors, rc, box)
    pairs = H.survivors(pos, donors, acceptors, (), rc, box)
    straddling = len(set(H.survivors(pos, donors, acceptors, (), rc, BOX)) - set(H.survivors(pos, donors, acceptors, (), rc, None)))
    name = 'three'
    dpar, apar = np.zeros((130, 0)), np.zeros((130, 0))
    e, f, context = one_force(len(pos), BOX, hbond_force(name, donors, acceptors, dpar, apar, (), method, rc), pos)
    stats = context._engine.hbond_stats(context._engine.entries[0].force)
    share = len(pairs) / 16900.0
    print('%s, rc = %.2f: %d of 16900 pairs survive (%.1f %%), %d only by the minimum image' % (method, rc, len(pairs), 100 * share, straddling))
    assert stats['survivors'] == len(pairs)
    assert {'none': share == 0.0, 'three-percent': 0.01 < share < 0.05, 'twenty-percent': 0.1 < share < 0.25, 'all': share == 1.0}[rate]
    if rate in ('three-percent', 'twenty-percent'):
        assert straddling > 100
    if not pairs:
        assert e == 0.0 and not f.any()
        return
    e_ref, f_ref, _ = one_force(len(pos), BOX, twin_force(name, donors, acceptors, dpar, apar, pairs, periodic), pos)
    assert_close(e, f, e_ref, f_ref, '%s, %s survival' % (method, rate))


# ------------------------------------------------------------------------------------ 4. exclusions
@pytest.mark.parametrize('count', (0, 1, 70))
def test_exclusions_on_one_donor(count):
    D, A, rc = 5, 200, 1.0
    pos, donors, acceptors = H.layout(D, A, 1.6, 41)
    assert H.margin_ok(pos, donors, acceptors, rc)
    inside = [a for d, a in H.survivors(pos, donors, acceptors, (), rc) if d == 2]
    assert len(inside) >= 70
    excl = [(2, a) for a in inside[:count]]
    pairs = H.survivors(pos, donors, acceptors, excl, rc)
    dpar, apar = np.zeros((D, 0)), np.zeros((A, 0))
    e, f, context = one_force(len(pos), None, hbond_force('three', donors, acceptors, dpar, apar, excl, 'CutoffNonPeriodic', rc), pos)
    assert context._engine.hbond_stats(context._engine.entries[0].force)['survivors'] == len(pairs)
    e_ref, f_ref, _ = one_force(len(pos), None, twin_force('three', donors, acceptors, dpar, apar, pairs), pos)
    assert_close(e, f, e_ref, f_ref, '%d exclusions on donor 2 (%d of its acceptors inside the cutoff)' % (count, len(inside)))
    if count == 1:
        # the excluded pair alone, inside the cutoff: nothing of it is left
        only = hbond_force('three', donors[2:3], acceptors[inside[0]:inside[0] + 1], dpar[:1], apar[:1], [(0, 0)], 'CutoffNonPeriodic', rc)
        e1, f1, _ = one_force(len(pos), None, only, pos)
        assert e1 == 0.0 and not f1.any()


# ------------------------------------------------------------------------------------ 5. shared atoms
def test_water_like_layout_sums_the_roles():
    """Each O is d2 of two donors and a1 of an acceptor; the pairs within a molecule are excluded."""
    edge, rc = 1.25, 0.35
    pos, donors, acceptors, excl = water(64, edge, 7, rc)
    box = np.full(3, edge)
    pairs = H.survivors(pos, donors, acceptors, excl, rc, box)
    dpar, apar = np.zeros((128, 0)), np.zeros((64, 0))
    e, f, context = one_force(len(pos), box, hbond_force('distance-angle', donors, acceptors, dpar, apar, excl, 'CutoffPeriodic', rc), pos)
    e_ref, f_ref, _ = one_force(len(pos), box, twin_force('distance-angle', donors, acceptors, dpar, apar, pairs, True), pos)
    assert_close(e, f, e_ref, f_ref, 'water-like, 64 molecules, %d pairs' % len(pairs))
    # an acceptor with all three slots, read by a dihedral over O-H...O-H
    e, f, context = one_force(len(pos), box, hbond_force('with-dihedral', donors, acceptors, dpar, apar, excl, 'CutoffPeriodic', rc), pos)
    e_ref, f_ref, _ = one_force(len(pos), box, twin_force('with-dihedral', donors, acceptors, dpar, apar, pairs, True), pos)
    assert_close(e, f, e_ref, f_ref, 'water-like with the dihedral, 64 molecules, %d pairs' % len(pairs))


# ------------------------------------------------------------------------------------ 6. determinism
def test_same_bits_and_exact_accumulation():
    edge, rc = 1.25, 0.35
    pos, donors, acceptors, excl = water(64, edge, 7, rc)
    force = hbond_force('distance-angle', donors, acceptors, np.zeros((128, 0)), np.zeros((64, 0)), excl, 'CutoffPeriodic', rc)
    e0, f0, context = one_force(len(pos), np.full(3, edge), force, pos)
    ctx, fid = context._engine.ctx, context._engine.entries[0].term_ids[0]
    e1, f1 = evaluate(ctx, fid, pos)
    e2, f2 = evaluate(ctx, fid, pos)
    _, f3 = evaluate(ctx, fid, pos, energy=False)
    assert e1 == e2 == e0 and np.array_equal(f1, f2) and np.array_equal(f1, f3) and np.array_equal(f1, f0)
    start = np.random.default_rng(5).normal(size=f1.shape) * 100.0
    _, f4 = evaluate(ctx, fid, pos, accumulate=True, start=start, energy=False)
    assert np.array_equal(f4, start + f1)
    ctx.check()


# ------------------------------------------------------------------------------------ 7. parameters
def test_parameters_and_their_updates():
    D, A, rc = 40, 70, 0.9
    pos, donors, acceptors = H.layout(D, A, 1.8, 51)
    assert H.margin_ok(pos, donors, acceptors, rc)
    name = 'parameters'
    dpar, apar = H.parameters(name, D, 'd', 5), H.parameters(name, A, 'a', 5)
    pairs = H.survivors(pos, donors, acceptors, (), rc)
    force = hbond_force(name, donors, acceptors, dpar, apar, (), 'CutoffNonPeriodic', rc)
    e, f, context = one_force(len(pos), None, force, pos)
    e_ref, f_ref, _ = one_force(len(pos), None, twin_force(name, donors, acceptors, dpar, apar, pairs), pos)
    assert_close(e, f, e_ref, f_ref, 'per-donor and per-acceptor parameters in one text, %d pairs' % len(pairs))
    # new per-donor and per-acceptor values and a new global: the same bits as a Context built with them
    dpar2, apar2 = H.parameters(name, D, 'd', 6), H.parameters(name, A, 'a', 6)
    for k in range(D):
        force.setDonorParameters(k, *[int(a) for a in donors[k]], [float(v) for v in dpar2[k]])
    for k in range(A):
        force.setAcceptorParameters(k, *[int(a) for a in acceptors[k]], [float(v) for v in apar2[k]])
    force.updateParametersInContext(context)
    context.setParameter('scale', 0.7)
    e_new, f_new = energy_forces(context)
    e_fresh, f_fresh, _ = one_force(len(pos), None, hbond_force(name, donors, acceptors, dpar2, apar2, (), 'CutoffNonPeriodic', rc, gvalues=dict(scale=0.7)), pos)
    print('after updateParametersInContext and setParameter: E = %.15g, fresh Context %.15g' % (e_new, e_fresh))
    assert e_new == e_fresh and np.array_equal(f_new, f_fresh) and e_new != e


# ------------------------------------------------------------------------------------ 8. integration
def thermal(n, mass, seed=2026):
    return np.random.default_rng(seed).normal(size=(n, 3)) * math.sqrt(2.494339 / mass)


def test_twenty_verlet_steps_against_the_explicit_bonds():
    D, A = 12, 12
    pos, donors, acceptors = H.layout(D, A, 1.2, 61)
    dpar, apar = np.zeros((D, 0)), np.zeros((A, 0))
    pairs = H.survivors(pos, donors, acceptors)
    xs = []
    for force in (hbond_force('three', donors, acceptors, dpar, apar), twin_force('three', donors, acceptors, dpar, apar, pairs)):
        system = bare_system(len(pos))
        system.addForce(force)
        integrator = openmm.VerletIntegrator(0.001)
        context = context_with(system, pos, integrator)
        context.setVelocities(thermal(len(pos), 12.0))
        integrator.step(20)
        xs.append(positions_of(context))
        context._engine.ctx.check()
    worst, moved = np.abs(xs[0] - xs[1]).max(), np.abs(xs[0] - pos).max()
    print('20 Verlet steps against the explicit bonds: max |dx| = %.3e nm, atoms moved up to %.3e nm' % (worst, moved))
    assert moved > 1e-3 and worst <= X_ABS


def water_hbonds(data, rc=0.35, group=0):
    """The hydrogen-bond force of a three-site water fixture: angle rows are (H, O, H)."""
    angles = np.asarray(data['angles'])
    donors = np.concatenate([np.stack([angles[:, 0], angles[:, 1], np.full(len(angles), -1)], axis=1),
                             np.stack([angles[:, 2], angles[:, 1], np.full(len(angles), -1)], axis=1)])
    acceptors = np.stack([angles[:, 1], angles[:, 0], angles[:, 2]], axis=1)
    m = len(angles)
    excl = [(k, k) for k in range(m)] + [(m + k, k) for k in range(m)]
    return hbond_force('distance-angle', donors, acceptors, np.zeros((2 * m, 0)), np.zeros((m, 0)), excl, 'CutoffPeriodic', rc, group=group)


def test_four_respa_steps_fusion_on_and_off(spcfw):
    results = []
    for fuse in (True, False):
        system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
        system = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        system.addForce(water_hbonds(spcfw, group=0))
        integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
        context = context_with(system, spcfw['positions'], integrator)
        context.setVelocities(np.random.default_rng(2026).normal(size=spcfw['positions'].shape) *
                              np.sqrt(2.494339 / spcfw['mass'])[:, None])
        context._engine.ctx.set_fuse_inner(fuse)
        assert [(type(e.force).__name__, e.group) for e in context._engine.entries if getattr(e, 'hbond', None)] == [('CustomHbondForce', 0)]
        integrator.step(4)
        results.append((positions_of(context), context._engine.ctx.run_stats()))
        context._engine.ctx.check()
    (x_on, stats_on), (x_off, stats_off) = results
    print('4 RESPA [4, 2, 1] steps: run statistics with fusion %s, without %s' % (stats_on, stats_off))
    assert np.array_equal(x_on, x_off) and stats_on['epilogues'] == 0 and stats_off['epilogues'] == 0
    assert np.abs(x_on - spcfw['positions']).max() > 1e-4


def test_minimisation_lowers_the_energy():
    edge, rc = 1.25, 0.35
    pos, donors, acceptors, excl = water(64, edge, 7, rc)
    system = bare_system(len(pos), np.full(3, edge))
    bonds = openmm.HarmonicBondForce()
    for m in range(64):
        bonds.addBond(3 * m, 3 * m + 1, 0.1, 2.0e5)
        bonds.addBond(3 * m, 3 * m + 2, 0.1, 2.0e5)
        bonds.addBond(3 * m + 1, 3 * m + 2, 0.1633, 5.0e4)
    system.addForce(bonds)
    # (a well deep enough that the start is far from converged: 200 kJ/mol at 0.19 nm)
    force = hbond_force('distance-angle', donors, acceptors, np.zeros((128, 0)), np.zeros((64, 0)), excl, 'CutoffPeriodic', rc,
                        gvalues=dict(eps=200.0, s=0.19))
    system.addForce(force)
    sim = app.Simulation(app.Topology(len(pos)), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(pos * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy(maxIterations=50)
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('minimisation: E %.8g -> %.8g kJ/mol' % (e0, e1))
    assert math.isfinite(e1) and e1 < e0
    sim.context._engine.ctx.check()


def test_langevin_middle_with_a_barostat(spcfw):
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    force = water_hbonds(spcfw, group=5)
    system.addForce(force)
    barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 10)
    barostat.setRandomNumberSeed(11)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(3)
    context = context_with(system, spcfw['positions'], integrator)
    context.setVelocitiesToTemperature(300.0, 5)
    integrator.step(50)
    state = context.getState(getEnergy=True, getPositions=True, groups={5})
    e_run = state.getPotentialEnergy()._value
    x = state.getPositions(asNumpy=True)._value
    vectors = state.getPeriodicBoxVectors()
    edges = np.array([vectors[k][k] if not hasattr(vectors[k][k], '_value') else vectors[k][k]._value for k in range(3)], dtype=np.float64)
    stats = context._engine.barostat_stats
    assert stats['attempts'] == 5 and math.isfinite(e_run) and np.isfinite(x).all()
    # a fresh Context at the final box and positions
    fresh = bare_system(len(x), edges)
    fresh.addForce(water_hbonds(spcfw, group=5))
    e_fresh, _ = energy_forces(context_with(fresh, x), groups={5})
    print('LangevinMiddle + barostat, 50 steps: %s; box %s -> %s; hydrogen-bond energy %.12g, fresh Context %.12g (rel %.2e)' % (
        stats, spcfw['box'], edges, e_run, e_fresh, abs(e_run - e_fresh) / abs(e_fresh)))
    assert e_fresh != 0.0 and abs(e_run - e_fresh) <= E_REL * abs(e_fresh)
    context._engine.ctx.check()


def test_free_space_system_runs():
    D, A = 6, 6
    pos, donors, acceptors = H.layout(D, A, 1.0, 71)
    system = bare_system(len(pos))
    nb = openmm.NonbondedForce()
    for _ in range(len(pos)):
        nb.addParticle(0.0, 0.2, 0.1)
    nb.setNonbondedMethod(nb.NoCutoff)
    system.addForce(nb)
    force = hbond_force('three', donors, acceptors, np.zeros((D, 0)), np.zeros((A, 0)), group=1)
    system.addForce(force)
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(system, pos, integrator)
    assert context._engine.free_space
    e, f = energy_forces(context, groups={1})
    e_ref, f_ref, _ = one_force(len(pos), None, twin_force('three', donors, acceptors, np.zeros((D, 0)), np.zeros((A, 0)),
                                                           H.survivors(pos, donors, acceptors)), pos)
    assert_close(e, f, e_ref, f_ref, 'free space, NoCutoff, 6 x 6')
    integrator.step(10)
    assert np.isfinite(positions_of(context)).all() and np.abs(positions_of(context) - pos).max() > 1e-6
    system.addForce(hbond_force('three', donors, acceptors, np.zeros((D, 0)), np.zeros((A, 0)), (), 'CutoffPeriodic', 0.3))
    with pytest.raises(atomsmm.InputError, match='periodic boundary'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 9. refusals at the C-ABI
def test_abi_refusals_name_the_cause():
    n = 6
    pos = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.3, 0.0, 0.0], [0.4, 0.0, 0.0], [0.3, 0.1, 0.0]]) + 1.0
    prog, _ = X.compile_hbond('distance(d1,a1)', [], [], [])
    ctx = B.HipContext(n, np.full(3, 2.0))
    nobox = B.HipContext(n, None)
    try:
        def create(c=ctx, kinds=(B.CVAR_DISTANCE,), slots=((0, 3),), donors=((0, 1, 2),), acceptors=((3, 4, 5),), dpar=None, apar=None, excl=None,
                   rc=0.0, periodic=False, prog=prog):
            donors, acceptors = np.array(donors, dtype=np.int32).reshape(-1, 3), np.array(acceptors, dtype=np.int32).reshape(-1, 3)
            return c.hbond_create(prog.code, prog.consts, [], list(kinds), [list(s) for s in slots], donors, acceptors,
                                  np.zeros((0, len(donors))) if dpar is None else dpar, np.zeros((0, len(acceptors))) if apar is None else apar,
                                  excl, rc=rc, periodic=periodic)
        many = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (32769, 1))
        with pytest.raises(B.HipError, match=r'amm_hbond_create: 32769 donors \(limit 32768\)'):
            create(donors=many)
        with pytest.raises(B.HipError, match=r'amm_hbond_create: 32769 acceptors \(limit 32768\)'):
            create(acceptors=many)
        with pytest.raises(B.HipError, match=r'amm_hbond_create: 17 geometric variables \(limit 16\)'):
            create(kinds=(B.CVAR_DISTANCE,) * 17, slots=((0, 3),) * 17)
        with pytest.raises(B.HipError, match=r'amm_hbond_create: 5 per-donor and 4 per-acceptor parameters \(limit 8 together\)'):
            create(dpar=np.zeros((5, 1)), apar=np.zeros((4, 1)))
        with pytest.raises(B.HipError, match='amm_hbond_create: atom index 6 of donor 0 is out of range'):
            create(donors=((0, 6, 2),))
        with pytest.raises(B.HipError, match='amm_hbond_create: atom index -1 of acceptor 0 is out of range'):
            create(acceptors=((-1, 4, 5),))
        with pytest.raises(B.HipError, match='amm_hbond_create: atom index -2 of acceptor 1 is out of range'):
            create(acceptors=((3, 4, 5), (3, -2, 5)))
        with pytest.raises(B.HipError, match=r'amm_hbond_create: exclusion 1 \(donor 1, acceptor 0\) is out of range'):
            create(excl=[(0, 0), (1, 0)])
        with pytest.raises(B.HipError, match=r'amm_hbond_create: exclusion 0 \(donor 0, acceptor -1\) is out of range'):
            create(excl=[(0, -1)])
        with pytest.raises(B.HipError, match='amm_hbond_create: CutoffPeriodic, but the context has no periodic box'):
            create(c=nobox, rc=0.5, periodic=True)
        with pytest.raises(B.HipError, match=r'amm_hbond_create: the cutoff 1\.10* exceeds half the shortest box edge \(2\.0*\)'):
            create(rc=1.1, periodic=True)
        with pytest.raises(B.HipError, match='amm_hbond_create: the text names d3, which donor 0 leaves at -1'):
            create(kinds=(B.CVAR_ANGLE,), slots=((2, 0, 3),), donors=((0, 1, -1),))
        with pytest.raises(B.HipError, match=r'amm_hbond_create: variable 0 names slot 6 beyond the pair \(6 slots: d1 d2 d3 a1 a2 a3\)'):
            create(slots=((0, 6),))
        with pytest.raises(B.HipError, match=r'amm_hbond_create: variable 0 has the kind 0 \(a hydrogen-bond text reads distance, angle and dihedral only\)'):
            create(kinds=(B.CVAR_X,))
        two = X.compile_hbond('distance(d1,a1)*distance(d2,a1)', [], [], [])[0]
        with pytest.raises(B.HipError, match=r'amm_hbond_create: variable index out of range'):
            create(prog=two)
        with_p = X.compile_hbond('k*distance(d1,a1)', ['k'], [], [])[0]
        with pytest.raises(B.HipError, match=r'amm_hbond_create: per-term parameter index out of range \(the force has 0\)'):
            create(prog=with_p)
        fid = create(donors=((0, 1, -1),), acceptors=((3, -1, -1),))
        e, f = evaluate(ctx, fid, pos)
        assert e == pytest.approx(0.3, rel=1e-12) and f[0, 0] == pytest.approx(1.0, rel=1e-12) and f[3, 0] == pytest.approx(-1.0, rel=1e-12)
        assert not f[[1, 2, 4, 5]].any() and ctx.hbond_stats(fid) == dict(scanned=1, survivors=1, launches=3, chunks=1)
        # the other families refuse the id, naming the type
        for call in (lambda: ctx.bonded_finalize(fid), lambda: ctx.bonded_release(fid), lambda: ctx.term_expr_set_globals(fid, []),
                     lambda: ctx.compound_set_globals(fid, []), lambda: ctx.compound_release(fid), lambda: ctx.custom_gb_set_globals(fid, []),
                     lambda: ctx.pair_set_params(fid, np.zeros(n), np.zeros(n), np.zeros(n)), lambda: ctx.pme_set_charges(fid, np.zeros(n))):
            with pytest.raises(B.HipError, match='AMM_FORCE_HBOND'):
                call()
        # ... and this family's another's, naming itself
        other, _ = X.compile_compound('distance(p1,p2)', 2, 'p', [], [])
        cid = ctx.compound_create(2, other.code, other.consts, [], [B.CVAR_DISTANCE], [[0, 1]], np.array([[0, 1]], dtype=np.int32), np.zeros((0, 1)))
        with pytest.raises(B.HipError, match=r'amm_hbond_stats: not the id of a hydrogen-bond force \(AMM_FORCE_HBOND\): force %d is a compound-bond force' % cid):
            ctx.hbond_stats(cid)
        with pytest.raises(B.HipError, match='amm_hbond_set_globals: the program reads 0 globals, 1 given'):
            ctx.hbond_set_globals(fid, [1.0])
        with pytest.raises(B.HipError, match='amm_hbond_set_params: the force has 1 donors of 0 parameters and 1 acceptors of 0, 1 x 2 and 1 x 0 given'):
            ctx.hbond_set_params(fid, np.zeros((2, 1)), 1, np.zeros((0, 1)), 1)
        with pytest.raises(B.HipError, match='amm_set_option: hbond_chunks is 0'):
            ctx.set_option('hbond_chunks', 513)
        # a periodic force whose box shrinks under it: refused at the evaluation, by name
        per = create(rc=0.9, periodic=True)
        ctx.set_box(np.full(3, 1.7))
        with pytest.raises(B.HipError, match=r'AMM_FORCE_HBOND\): the cutoff 0\.90* exceeds half the shortest box edge'):
            evaluate(ctx, per, pos)
        ctx.hbond_release(fid)
        with pytest.raises(B.HipError, match='amm_hbond_release: not the id of a hydrogen-bond force'):
            ctx.hbond_release(fid)
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, pos)
        ctx.check()
    finally:
        ctx.close()
        nobox.close()
