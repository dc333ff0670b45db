"""GPU tests of the Gay-Berne force (csrc/gayberne.hip): ellipsoids whose frames other particles define, the torque returned as forces
on those particles.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|, against the 50-digit checker of
tests/gayberne_cases.py, whose forces are central differences of its energy -- no hand derivation on that side.  Small cases are
evaluated by the checker here, once; the cases of 63 ellipsoids and more are its recorded answers (tests/golden/data/gayberne_*.npz).
Two conditions are asserted on the CHECKER's numbers for every case: every interacting pair has (h12 + sigma) / sigma >= 0.75, and
every case of several pairs has a pair with rho > 1 -- no case hides in the flat tail or blows up in an overlap.  Every test prints
its own deviation; DESIGN.md 3.GY has the worst ones measured on an MI355X."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import gayberne_cases as GC  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import engine as E  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402

E_REL, F_REL = 1e-10, 1e-9
MARKER, force_of = GC.MARKER, GC.force_of


# ------------------------------------------------------------------------------------ the cases
def unit_of(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def two_bodies(bodies, separation, target=0.9):
    """bodies: two of (sigma, eps, shape, x axis or None, y direction or None); the centres lie at -+ separation / 2 and are then
    settled to the contact ratio `target`.  A body's markers come before it: 0.1 nm behind the centre along x, 0.12 nm along the y
    direction (which need not be perpendicular to x)."""
    parts, pos, rides = [], [], []
    for k, (sigma, eps, shape, xdir, ydir) in enumerate(bodies):
        centre = (k - 0.5) * np.asarray(separation, dtype=np.float64)
        first = len(parts)
        me = first + (xdir is not None) + (ydir is not None)
        if xdir is not None:
            parts.append(MARKER)
            pos.append(centre - 0.1 * unit_of(xdir))
        if ydir is not None:
            parts.append(MARKER)
            pos.append(centre - 0.12 * unit_of(ydir))
        parts.append((sigma, eps, first if xdir is not None else -1, first + 1 if ydir is not None else -1) + tuple(shape))
        pos.append(centre)
        rides += [me] * (me - first + 1)
    spec = GC.spec_of(parts)
    return spec, GC.settle(spec, np.array(pos), rides, target)


def sixty_degrees(xdir, seed):
    """A direction 60 degrees off xdir: d2 is far from perpendicular to d1, so moving the x-particle rolls the frame."""
    x = unit_of(xdir)
    side = unit_of(np.cross(x, np.random.default_rng(seed).normal(size=3)))
    return 0.5 * x + math.sqrt(0.75) * side


def cutoff_case(switch):
    """A-B in contact, C inside the switching interval of A and of B, D just beyond the cutoff of A (and beyond that of B and C)."""
    rng = np.random.default_rng(7)
    centres = np.array([[0.0, 0.0, 0.0], [0.28, 0.0, 0.0], [0.0, 0.8, 0.0], [0.0, 0.0, -0.9005]])
    parts, pos = [], []
    for k, c in enumerate(centres):
        axis = unit_of(np.array([0.0, 0.0, 1.0]) + 0.15 * rng.normal(size=3))
        parts += [MARKER, (GC.SIGMA, GC.EPS + 0.2 * k, 2 * k, -1) + GC.UNIAXIAL]
        pos += [c - 0.1 * axis, c]
    return GC.spec_of(parts, method=GC.CUTOFF_NONPERIODIC, cutoff=0.9, switch=switch), np.array(pos)


def periodic_case():
    """Box 2 nm, cutoff 0.9: A and B in contact across the x face; C at the y face with its marker on the other side; D next to C
    through that face; E biaxial at a corner with both markers across faces."""
    L = 2.0
    z, y = np.array([0.05, -0.08, 1.0]), np.array([0.06, 1.0, 0.04])
    bodies = [((1.9, 0.5, 0.5), z, None, GC.UNIAXIAL), ((0.18, 0.5, 0.5), z, None, GC.UNIAXIAL), ((1.0, 1.95, 0.5), -y, None, GC.UNIAXIAL),
              ((1.05, 0.5, 0.5), y, None, GC.UNIAXIAL), ((1.97, 1.96, 1.95), (-1.0, -0.9, -0.2), (0.3, -1.0, -1.0), GC.BIAXIAL)]
    parts, pos = [], []
    for k, (c, xdir, ydir, shape) in enumerate(bodies):
        c = np.array(c)
        first = len(parts)
        parts.append(MARKER)
        pos.append((c - 0.1 * unit_of(xdir)) % L)
        if ydir is not None:
            parts.append(MARKER)
            pos.append((c - 0.12 * unit_of(ydir)) % L)
        parts.append((GC.SIGMA, GC.EPS + 0.1 * k, first, first + 1 if ydir is not None else -1) + shape)
        pos.append(c)
    pos = np.array(pos)
    assert np.abs(pos[0] - pos[1]).max() < 0.2 and abs(pos[5, 1] - pos[4, 1]) > 1.0          # (A's marker is next to A, C's across the face)
    return GC.spec_of(parts, method=GC.CUTOFF_PERIODIC, cutoff=0.9, switch=0.75, box=(L, L, L)), pos


def shared_markers():
    """Particle 0 is the x-particle of ellipsoids 1, 2, 3 and the y-particle of ellipsoid 4, whose x-particle is ellipsoid 1."""
    parts = [MARKER, (GC.SIGMA, 1.2, 0, -1) + GC.UNIAXIAL, (GC.SIGMA, 1.5, 0, -1) + GC.OBLATE, (0.32, 1.8, 0, -1) + GC.UNIAXIAL,
             (GC.SIGMA, 1.1, 1, 0) + GC.BIAXIAL]
    pos = np.array([[0.0, 0.0, 0.0], [0.42, 0.02, 0.0], [-0.12, 0.40, 0.03], [-0.10, -0.22, 0.38], [0.40, 0.42, 0.30]])
    spec = GC.spec_of(parts)
    return spec, GC.settle(spec, pos, list(range(5)), 0.9)


def some_exceptions():
    """Six ellipsoids: an override, an epsilon-0 exclusion, and an exception that brings a particle with epsilon 0 into the scan."""
    spec, pos, ell = GC.fluid(6, 61, biaxial_every=3)
    spec['particles'][ell[5]] = (GC.SIGMA, 0.0) + spec['particles'][ell[5]][2:]
    spec['exceptions'] = [(ell[0], ell[1], 0.29, 2.2), (ell[2], ell[1], 0.3, 0.0), (ell[5], ell[3], 0.31, 1.7)]
    return spec, pos


Z, XA = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
U1, U2 = (GC.SIGMA, 1.5, GC.UNIAXIAL), (0.32, 1.1, GC.UNIAXIAL)
CASES = {
    'sphere-sphere': lambda: two_bodies([(0.3, 1.5, GC.SPHERE, None, None), (0.34, 0.9, (0.34, 0.34, 0.34, 1.0, 1.0, 1.0), None, None)], (0.3, 0.1, -0.2)),
    'sphere-uniaxial': lambda: two_bodies([(0.3, 1.5, GC.SPHERE, None, None), U2 + ((0.3, 0.5, 1.0), None)], (0.3, 0.1, -0.2)),
    'side-by-side': lambda: two_bodies([U1 + (Z, None), U2 + (Z, None)], (0.3, 0.0, 0.0)),
    'end-to-end': lambda: two_bodies([U1 + (Z, None), U2 + (Z, None)], (0.0, 0.0, 0.5)),
    'tee': lambda: two_bodies([U1 + (Z, None), U2 + (XA, None)], (0.4, 0.0, 0.0)),
    'skew': lambda: two_bodies([U1 + ((0.3, -0.8, 0.5), None), U2 + ((-0.6, 0.2, 0.7), None)], (0.3, 0.25, -0.2)),
    'oblate-prolate': lambda: two_bodies([(0.3, 1.5, GC.OBLATE, (0.2, 0.9, 0.1), None), U2 + ((-0.6, 0.2, 0.7), None)], (0.25, 0.3, 0.2)),
    'biaxial-roll': lambda: two_bodies([(0.3, 1.5, GC.BIAXIAL, (0.3, -0.8, 0.5), sixty_degrees((0.3, -0.8, 0.5), 1)),
                                        (0.31, 1.2, GC.BIAXIAL, (-0.6, 0.2, 0.7), sixty_degrees((-0.6, 0.2, 0.7), 2))], (0.3, 0.25, -0.2)),
    'n1': lambda: GC.fluid(1, 101)[:2], 'n2': lambda: GC.fluid(2, 102, biaxial_every=1)[:2],
    'cutoff': lambda: cutoff_case(None), 'cutoff-switch': lambda: cutoff_case(0.7),
    'periodic': periodic_case, 'shared-markers': shared_markers, 'some-exceptions': some_exceptions,
}
TWO_BODY = ['sphere-sphere', 'sphere-uniaxial', 'side-by-side', 'end-to-end', 'tee', 'skew', 'oblate-prolate', 'biaxial-roll']
LIVE = TWO_BODY + ['n1', 'n2', 'cutoff', 'cutoff-switch', 'periodic', 'shared-markers', 'some-exceptions']
ALL = LIVE + sorted(GC.RECORDED)
SINGLE_PAIR = set(TWO_BODY) | {'n1', 'n2'}


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(spec, positions, the checker's answer): computed or loaded once, never changed."""
    if name in GC.RECORDED:
        spec, pos, _, out = GC.recorded(name)
        return spec, pos, out
    spec, pos = CASES[name]()
    pos.setflags(write=False)
    out = GC.evaluate(spec, pos)
    out['forces'].setflags(write=False)
    return spec, pos, out


def make(ctx, spec):
    """The force at the C interface, from the tables the engine builds."""
    tab = E.gayberne_tables(force_of(spec), len(spec['particles']))
    rc = 0.0 if spec['method'] == GC.NO_CUTOFF else spec['cutoff']
    rs = spec['switch'] if spec['method'] != GC.NO_CUTOFF and spec['switch'] is not None else -1.0
    return ctx.gayberne_create(tab['active'], tab['axes'], tab['par'], tab['ex_ptr'], tab['ex_col'], tab['ex_par'], tab['rev_ptr'], tab['rev_src'],
                               rc=rc, rs=rs, periodic=spec['method'] == GC.CUTOFF_PERIODIC)


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')            # (a copy: the cases are read-only)


def evaluate(ctx, fid, pos, accumulate=False, start=None, energy=True):
    f = dev(np.full((len(pos), 3), np.nan) if start is None else start)       # (every row has to be written)
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, dev(pos), f, accumulate=accumulate, energy=e)
    ctx.synchronize()
    return (e.item() if energy else None), f.cpu().numpy()


@functools.lru_cache(maxsize=None)
def run_of(name):
    """One context per case: two evaluations with the energy, one without, one that accumulates onto a given start."""
    spec, pos, _ = case_of(name)
    ctx = B.HipContext(len(pos), None if spec['box'] is None else np.array(spec['box']))
    try:
        fid = make(ctx, spec)
        e1, f1 = evaluate(ctx, fid, pos)
        e2, f2 = evaluate(ctx, fid, pos)
        _, f3 = evaluate(ctx, fid, pos, energy=False)
        start = np.random.default_rng(99).normal(size=pos.shape)
        _, f4 = evaluate(ctx, fid, pos, accumulate=True, start=start, energy=False)
        stats = ctx.gayberne_stats(fid)
        ctx.check()
    finally:
        ctx.close()
    return dict(e=e1, f=f1, again=(e2, f2), no_energy=f3, start=start, accumulated=f4, stats=stats)


def assert_close(e, f, out, what):
    e_ref, f_ref = out['energy'], out['forces']
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (checker %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g; closest contact %.3f, largest rho %.3f, %d pairs' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale,
           out['min_ratio'], out['max_rho'], out['n_pairs']))
    assert np.isfinite(e) and np.isfinite(f).all()
    assert abs(e - e_ref) <= E_REL * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


# ------------------------------------------------------------------------------------ 1. the kernels against the checker
@pytest.mark.parametrize('name', ALL)
def test_the_case_is_neither_flat_nor_an_overlap(name):
    """On the checker's numbers alone."""
    spec, pos, out = case_of(name)
    print('%s: %d pairs, closest contact (h12 + sigma) / sigma = %.4f, largest rho = %.4f' % (name, out['n_pairs'], out['min_ratio'], out['max_rho']))
    if name == 'n1':
        assert out['n_pairs'] == 0 and out['energy'] == 0.0
        return
    assert out['n_pairs'] >= 1 and out['min_ratio'] >= 0.75
    if name not in SINGLE_PAIR:
        assert out['n_pairs'] > 1 and out['max_rho'] > 1.0
    assert np.abs(out['forces']).max() > 1.0


@pytest.mark.parametrize('name', ALL)
def test_energy_and_forces_match_the_checker(name):
    spec, pos, out = case_of(name)
    run = run_of(name)
    assert_close(run['e'], run['f'], out, name)
    # each pair is counted from both sides
    assert run['stats']['survivors'] == 2 * out['n_pairs']
    n_act = run['stats']['active']
    assert run['stats']['scanned'] == n_act * (n_act - 1)


def test_the_roll_case_rolls():
    """The biaxial pair: d2 lies sixty degrees off d1 on both ellipsoids, so moving an x-particle also rolls the frame about x^ -- a
    transfer of torque without that term fails test_energy_and_forces_match_the_checker[biaxial-roll]."""
    spec, pos, out = case_of('biaxial-roll')
    for x, y, me in ((0, 1, 2), (3, 4, 5)):
        assert spec['particles'][me][2:4] == (x, y)
        d1, d2 = pos[me] - pos[x], pos[me] - pos[y]
        cosine = d1 @ d2 / np.linalg.norm(d1) / np.linalg.norm(d2)
        assert cosine == pytest.approx(0.5, abs=1e-9)
    assert np.abs(out['forces'][[0, 1, 3, 4]]).min(axis=1).max() > 0.0 and np.abs(out['forces'][[1, 4]]).max() > 1e-2 * np.abs(out['forces']).max()


@pytest.mark.parametrize('name', ALL)
def test_evaluation_modes(name):
    spec, pos, out = case_of(name)
    run = run_of(name)
    e2, f2 = run['again']
    assert e2 == run['e'] and np.array_equal(f2, run['f'])                          # the same bits
    assert np.array_equal(run['no_energy'], run['f'])                               # without the energy
    assert np.isfinite(run['f']).all()                                              # every row written over the NaN it started from
    # onto a random start: one rounding of the sum per component
    want = run['start'] + run['f']
    assert np.abs(run['accumulated'] - want).max() <= 2.0 ** -52 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('name', [n for n in ALL if n != 'periodic'])
def test_forces_and_torques_sum_to_zero(name):
    spec, pos, _ = case_of(name)
    f = run_of(name)['f']
    total = np.abs(f).sum()
    net, torque = np.abs(f.sum(axis=0)).max(), np.abs(np.cross(pos, f).sum(axis=0)).max()
    print('%s: |sum F| = %.3e, |sum r x F| = %.3e, sum|F| = %.6g' % (name, net, torque, total))
    assert net <= 1e-9 * total and torque <= 1e-9 * total


def test_row_and_tile_edges_take_the_paths_they_are_meant_for():
    """1, 2, 63, 64, 65, 129 and 257 active rows: below, at and above one batch of 64 columns, and rows split into chunks."""
    want = {'n1': 1, 'n2': 2, 'n63': 63, 'n64': 64, 'n65': 65, 'n129': 129, 'n257': 257, 'exc72': 72}
    for name, rows in want.items():
        stats = run_of(name)['stats']
        batches = (rows + 63) // 64
        print('%s: %s' % (name, stats))
        assert stats['active'] == rows and stats['chunks'] == batches              # (4096 / rows >= batches here: one batch per chunk)
        assert stats['launches'] == 4 * 4
    spec, pos, _ = case_of('n64')
    assert len(pos) > 2 * 64                                                        # biaxial ones among them: second markers


# ------------------------------------------------------------------------------------ 2. through the Python API
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


@pytest.mark.parametrize('name', ['shared-markers', 'cutoff-switch', 'periodic'])
def test_through_the_engine(name):
    spec, pos, out = case_of(name)
    system = bare_system(len(pos), spec['box'] if spec['method'] == GC.CUTOFF_PERIODIC else None)
    force = force_of(spec)
    system.addForce(force)
    context = context_with(system, pos)
    e, f = energy_forces(context)
    assert_close(e, f, out, 'GayBerneForce in a Context (%s)' % name)
    stats = context._engine.gayberne_stats(force)
    assert stats['survivors'] == 2 * out['n_pairs']
    context._engine.ctx.check()


def test_the_lennard_jones_limit_agrees_with_a_nonbonded_force():
    """Spheres with sx = sy = sz = sigma and e = 1 are Lennard-Jones particles (sigma12 = sigma needs ONE diameter; the well depths
    differ): the same numbers as a NonbondedForce without charges, both through the engine, NoCutoff, an override and an exclusion."""
    rng = np.random.default_rng(12)
    n = 40
    grid = np.array([(a, b, c) for a in range(4) for b in range(4) for c in range(3)], dtype=np.float64)[:n]
    pos = grid * 0.34 + rng.uniform(-0.03, 0.03, size=(n, 3))
    s = 0.31
    eps = 0.5 + rng.random(n)
    gb, nb = openmm.GayBerneForce(), openmm.NonbondedForce()
    for e in eps:
        gb.addParticle(s, e, -1, -1, s, s, s, 1.0, 1.0, 1.0)
        nb.addParticle(0.0, s, e)
    gb.addException(0, 1, s, 0.8)
    nb.addException(0, 1, 0.0, s, 0.8)
    gb.addException(2, 3, s, 0.0)
    nb.addException(2, 3, 0.0, s, 0.0)
    results = []
    for force in (gb, nb):
        system = bare_system(n)
        system.addForce(force)
        context = context_with(system, pos)
        results.append(energy_forces(context))
        context._engine.ctx.check()
    (e_gb, f_gb), (e_nb, f_nb) = results
    top = np.abs(f_nb).max()
    print('Lennard-Jones limit: E = %.15g against %.15g (rel %.2e); max|dF| = %.2e of max|F| = %.6g' %
          (e_gb, e_nb, abs(e_gb - e_nb) / abs(e_nb), np.abs(f_gb - f_nb).max() / top, top))
    assert abs(e_gb - e_nb) <= E_REL * abs(e_nb)
    assert np.abs(f_gb - f_nb).max() <= F_REL * top


def test_update_parameters_in_context_matches_a_fresh_context():
    spec, pos = some_exceptions()
    system = bare_system(len(pos))
    force = force_of(spec)
    system.addForce(force)
    context = context_with(system, pos)
    before = energy_forces(context)
    ell = [i for i, p in enumerate(spec['particles']) if p[2] >= 0]
    new = list(spec['particles'][ell[1]])
    new[0], new[1], new[4] = 0.31, 2.4, 0.55                       # sigma, epsilon, sx
    force.setParticleParameters(ell[1], *new)
    force.setExceptionParameters(0, ell[0], ell[1], 0.3, 1.3)
    force.updateParametersInContext(context)
    after = energy_forces(context)
    spec2 = dict(spec, particles=list(spec['particles']), exceptions=list(spec['exceptions']))
    spec2['particles'][ell[1]] = tuple(new)
    spec2['exceptions'][0] = (ell[0], ell[1], 0.3, 1.3)
    fresh_system = bare_system(len(pos))
    fresh_system.addForce(force_of(spec2))
    fresh = energy_forces(context_with(fresh_system, pos))
    print('updateParametersInContext: E %.12g -> %.12g (fresh Context %.12g)' % (before[0], after[0], fresh[0]))
    assert abs(after[0] - before[0]) > 1e-3 * abs(before[0])
    assert after[0] == fresh[0] and np.array_equal(after[1], fresh[1])
    assert_close(after[0], after[1], GC.evaluate(spec2, pos), '... against the checker')
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 3. 64 ellipsoids bonded to their markers
def bonded_fluid():
    """64 ellipsoids (every fourth biaxial) under CutoffNonPeriodic with a switch, each bonded to its markers by harmonic bonds and,
    with two markers, a harmonic angle -- the Gay-Berne force alone in group 3."""
    spec, pos, ell = GC.fluid(64, 264, biaxial_every=4)
    spec = dict(spec, method=GC.CUTOFF_NONPERIODIC, cutoff=0.6, switch=0.5)
    bonds, angles = openmm.HarmonicBondForce(), openmm.HarmonicAngleForce()
    for i in ell:
        xp, yp = spec['particles'][i][2:4]
        bonds.addBond(i, xp, float(np.linalg.norm(pos[i] - pos[xp])), 2.0e4)
        if yp >= 0:
            bonds.addBond(i, yp, float(np.linalg.norm(pos[i] - pos[yp])), 2.0e4)
            a, b = pos[xp] - pos[i], pos[yp] - pos[i]
            angles.addAngle(xp, i, yp, float(np.arccos(a @ b / np.linalg.norm(a) / np.linalg.norm(b))), 400.0)
    return spec, pos, ell, bonds, angles


def bonded_context(integrator, gb_group, push=0.0):
    spec, pos, ell, bonds, angles = bonded_fluid()
    system = bare_system(len(pos))
    bonds.setForceGroup(0)
    angles.setForceGroup(0)
    force = force_of(spec)
    force.setForceGroup(gb_group)
    for f in (bonds, angles, force):
        system.addForce(f)
    start = pos + push * np.random.default_rng(5).normal(size=pos.shape)
    return spec, start, force, context_with(system, start, integrator)


def thermal(n, mass, seed=5, kT=2.494339):
    return np.random.default_rng(seed).normal(size=(n, 3)) * math.sqrt(kT / mass)


def test_get_state_isolates_the_force_and_minimisation_lowers_the_energy():
    spec, pos, force, context = bonded_context(openmm.VerletIntegrator(0.001), 3, push=0.004)
    out = GC.evaluate(spec, pos)
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0
    e3, f3 = energy_forces(context, groups={3})
    assert_close(e3, f3, out, 'getState(groups={3}): the Gay-Berne force alone')
    e0, _ = energy_forces(context, groups={0})
    e_all, _ = energy_forces(context)
    assert e0 > 0.0 and abs(e_all - (e0 + e3)) <= 1e-12 * max(abs(e_all), abs(e0))
    openmm.LocalEnergyMinimizer.minimize(context, 1.0, 50)                          # (what Simulation.minimizeEnergy calls)
    e_min, _ = energy_forces(context)
    print('minimisation: %.6g -> %.6g kJ/mol' % (e_all, e_min))
    assert math.isfinite(e_min) and e_min < e_all
    context._engine.ctx.check()


def test_a_verlet_step_agrees_with_the_checker_at_the_final_positions():
    integrator = openmm.VerletIntegrator(0.001)
    spec, pos, force, context = bonded_context(integrator, 3)
    context.setVelocities(thermal(len(pos), 12.0))
    integrator.step(4)
    x = positions_of(context)
    out = GC.evaluate(spec, x)
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0
    e3, f3 = energy_forces(context, groups={3})
    moved = np.abs(x - pos).max()
    print('4 Verlet steps: particles moved up to %.3e nm' % moved)
    assert moved > 1e-4
    assert_close(e3, f3, out, 'after 4 Verlet steps')
    context._engine.ctx.check()


def test_a_respa_step_with_the_force_in_the_outer_group_agrees_with_the_checker():
    """RESPA [2, 1]: bonds and angles in the inner group 0, the Gay-Berne force alone in group 1."""
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    spec, pos, force, context = bonded_context(integrator, 1)
    context.setVelocities(thermal(len(pos), 12.0))
    integrator.step(4)
    x = positions_of(context)
    out = GC.evaluate(spec, x)
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0
    e1, f1 = energy_forces(context, groups={1})
    moved = np.abs(x - pos).max()
    print('4 RESPA [2, 1] steps: particles moved up to %.3e nm' % moved)
    assert moved > 1e-4
    assert_close(e1, f1, out, 'after 4 RESPA steps')
    context._engine.ctx.check()


def test_a_virtual_site_as_axis_particle():
    """The x-particle of the first ellipsoid of the skew pair is a TwoParticleAverageSite of two added particles: the torque it
    takes is spread to them, the total force stays zero."""
    spec, pos, out = case_of('skew')
    n = len(pos)
    pos = np.concatenate([pos, [pos[0] + [0.05, -0.02, 0.03], pos[0] - np.array([0.05, -0.02, 0.03]) * 0.3 / 0.7]])
    spec = dict(spec, particles=spec['particles'] + [MARKER, MARKER])
    system = bare_system(n + 2)
    system.setParticleMass(0, 0.0)
    system.setVirtualSite(0, openmm.TwoParticleAverageSite(n, n + 1, 0.3, 0.7))
    system.addForce(force_of(spec))
    context = context_with(system, pos)
    context.computeVirtualSites()
    x = positions_of(context)
    assert np.abs(x[0] - pos[0]).max() <= 2e-15
    ref = GC.evaluate(spec, x)
    want = ref['forces'].copy()
    want[n] += 0.3 * want[0]
    want[n + 1] += 0.7 * want[0]
    want[0] = 0.0
    e, f = energy_forces(context)
    scale = np.abs(want).max()
    assert np.abs(ref['forces'][0]).max() > 1e-2 * scale and not f[0].any()
    assert_close(e, f, dict(ref, forces=want), 'a virtual site as the x-particle')
    assert np.abs(f.sum(axis=0)).max() <= F_REL * scale
    context._engine.ctx.check()


def test_constant_pressure_steps_follow_the_box():
    """27 ellipsoids bonded to their markers under CutoffPeriodic with a MonteCarloBarostat at every second step: the force reads
    the box of the moment (frames and pairs by its minimum images), and agrees with the checker in the final box."""
    spec, pos, ell = GC.fluid(27, 327, biaxial_every=4)
    extent = float((pos[ell].max(axis=0) - pos[ell].min(axis=0)).max())
    edge = extent + 1.1 * extent / 2                                      # 3 x 3 x 3: the images as far away as the neighbours, and a bit
    pos = pos - pos[ell].min(axis=0) + 0.25 * extent
    spec = dict(spec, method=GC.CUTOFF_PERIODIC, cutoff=0.6, switch=0.5, box=(edge, edge, edge))
    bonds = openmm.HarmonicBondForce()
    for i in ell:
        for m in spec['particles'][i][2:4]:
            if m >= 0:
                bonds.addBond(i, m, float(np.linalg.norm(pos[i] - pos[m])), 2.0e4)
    system = bare_system(len(pos), spec['box'])
    system.addForce(bonds)
    force = force_of(spec)
    force.setForceGroup(2)
    system.addForce(force)
    barostat = openmm.MonteCarloBarostat(2000.0 * unit.bar, 300.0 * unit.kelvin, 2)
    barostat.setRandomNumberSeed(11)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(3)
    context = context_with(system, pos, integrator)
    context.setVelocities(thermal(len(pos), 12.0))
    integrator.step(12)
    state = context.getState(getPositions=True)
    x = state.getPositions(asNumpy=True)._value
    box = tuple(float(v._value[k]) for k, v in enumerate(state.getPeriodicBoxVectors()))
    print('12 NPT steps: box edge %.6f -> %.6f nm' % (edge, box[0]))
    assert np.isfinite(x).all()
    out = GC.evaluate(dict(spec, box=box), x)
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0 and out['n_pairs'] > 27
    e2, f2 = energy_forces(context, groups={2})
    assert_close(e2, f2, out, 'after 12 steps at constant pressure')
    # and a box set by hand, whatever the barostat accepted: the same positions, other images
    wider = tuple(1.04 * v for v in box)
    context.setPeriodicBoxVectors((wider[0], 0, 0), (0, wider[1], 0), (0, 0, wider[2]))
    out = GC.evaluate(dict(spec, box=wider), x)
    e2w, f2w = energy_forces(context, groups={2})
    assert_close(e2w, f2w, out, 'in a box 4 % wider')
    assert abs(e2w - e2) > 1e-6 * abs(e2)
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 4. refusals at the C-ABI
def test_abi_refusals_name_the_family():
    spec, pos, _ = case_of('shared-markers')
    n = len(pos)
    tab = E.gayberne_tables(force_of(spec), n)
    order = ('active', 'axes', 'par', 'ex_ptr', 'ex_col', 'ex_par', 'rev_ptr', 'rev_src')
    ctx = B.HipContext(n, None)
    try:
        def broken(**change):
            t = {k: np.array(v) for k, v in tab.items()}
            for key, (index, value) in change.items():
                t[key][index] = value
            return [t[k] for k in order]
        for args, kw in ((broken(active=(0, 7)), {}), (broken(active=(1, 1)), {}), (broken(axes=((0, 0), 9)), {}), (broken(axes=((0, 0), 1)), {}),
                         (broken(par=((0, 3), 0.31)), {}), (broken(rev_src=(0, 1)), {}), (broken(rev_ptr=(n, 3)), {}),
                         (broken(), dict(rc=0.5, rs=0.5)), (broken(), dict(rc=0.5, periodic=True))):
            with pytest.raises(B.HipError, match='amm_gayberne_create: .*AMM_FORCE_GAYBERNE'):
                ctx.gayberne_create(*args, **kw)
        fid = make(ctx, spec)
        before = evaluate(ctx, fid, pos)
        # a refused change leaves the force as it was
        bad = tab['par'].copy()
        bad[0, 3] = 0.31                                              # sy != sz without a y-particle
        with pytest.raises(B.HipError, match='amm_gayberne_set_params: no y-particle of active row 0.*AMM_FORCE_GAYBERNE'):
            ctx.gayberne_set_params(fid, bad, tab['ex_par'])
        with pytest.raises(B.HipError, match='amm_gayberne_set_params: the force has 4 active particles and 0 exception entries, 3 and 0 given'):
            ctx.gayberne_set_params(fid, tab['par'][:3], tab['ex_par'])
        after = evaluate(ctx, fid, pos)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        # an id of another family
        prog = X.compile_term('x*x', ('x', 'y', 'z'), [], [])
        rows = np.full((n, 4), -1, dtype=np.int32)
        rows[:, 0] = np.arange(n)
        other = ctx.term_expr_create(B.TERM_EXTERNAL, prog.code, prog.consts, [], rows, np.zeros((0, 1)))
        with pytest.raises(B.HipError) as err:
            ctx.gayberne_stats(other)
        assert str(err.value) == ('amm_gayberne_stats: not the id of a Gay-Berne force (AMM_FORCE_GAYBERNE): force %d is a term-expression force '
                                  '(AMM_FORCE_TERM_EXPR: amm_term_expr_*)' % other)
        with pytest.raises(B.HipError, match=r'amm_term_expr_release: not a term-expression force id: force %d is a Gay-Berne force '
                                             r'\(AMM_FORCE_GAYBERNE: amm_gayberne_\*\)' % fid):
            ctx.term_expr_release(fid)
        # several ranks
        with pytest.raises(B.HipError) as err:
            B._chk(B.lib().amm_set_slice(ctx.h, 0, 2))
        assert str(err.value) == 'amm_set_slice: a Gay-Berne force (AMM_FORCE_GAYBERNE) runs on a single rank'
        # released: its own entry points refuse it bare, the evaluation as a released id
        ctx.gayberne_release(fid)
        with pytest.raises(B.HipError) as err:
            ctx.gayberne_release(fid)
        assert str(err.value) == 'amm_gayberne_release: not the id of a Gay-Berne force (AMM_FORCE_GAYBERNE)'
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, pos)
        B._chk(B.lib().amm_set_slice(ctx.h, 0, 2))                    # nothing single-rank is left
        B._chk(B.lib().amm_set_slice(ctx.h, 0, 1))
        ctx.check()
    finally:
        ctx.close()
