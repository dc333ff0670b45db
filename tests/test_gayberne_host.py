"""CPU tests of GayBerneForce: the object model, what the engine refuses and what it hands to the library -- the compacted particles,
the exceptions' CSR and the reverse table of the axis particles, on the call recorder -- and the checker the GPU tests compare the
kernels with (tests/gayberne_cases.py) against closed forms that follow from the definition, against its own invariances and against
the recorded answers of the large cases."""
import math

import mpmath
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import gayberne_cases as GC
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.utils import InputError
from fake_backend import RecordingContext


class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.gaybernes = []

    def gayberne_create(self, active, axes, par, ex_ptr, ex_col, ex_par, rev_ptr, rev_src, rc=0.0, rs=-1.0, periodic=False):
        fid = self._new()
        self.gaybernes.append(dict(id=fid, active=np.array(active), axes=np.array(axes), par=np.array(par), ex_ptr=np.array(ex_ptr),
                                   ex_col=np.array(ex_col), ex_par=np.array(ex_par), rev_ptr=np.array(rev_ptr), rev_src=np.array(rev_src),
                                   rc=rc, rs=rs, periodic=periodic))
        return fid

    def gayberne_set_params(self, fid, par, ex_par):
        self.calls.append(('gayberne_set_params', fid, np.array(par), np.array(ex_par)))

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


def bare_system(n, box=3.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.0)
    if box:
        system.setDefaultPeriodicBoxVectors((box, 0, 0), (0, box, 0), (0, 0, box))
    return system


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


MARKER, force_of = GC.MARKER, GC.force_of


def small_spec():
    """0 marker, 1 uniaxial on 0, 2 sphere, 3 marker, 4 biaxial on (0, 3), 5 sphere with epsilon 0 that an exception brings in,
    6 a sphere with epsilon 0 that nothing brings in."""
    return GC.spec_of([MARKER, (0.3, 1.0, 0, -1) + GC.UNIAXIAL, (0.32, 2.0, -1, -1) + GC.SPHERE, MARKER, (0.3, 1.5, 0, 3) + GC.BIAXIAL,
                       (0.3, 0.0, -1, -1) + GC.SPHERE, (0.3, 0.0, -1, -1) + GC.SPHERE],
                      exceptions=[(5, 1, 0.31, 0.7), (4, 2, 0.3, 0.0), (6, 2, 0.3, 0.0)])


# ------------------------------------------------------------------------------------ the object model
def test_api_round_trips():
    force = openmm.GayBerneForce()
    assert (force.NoCutoff, force.CutoffNonPeriodic, force.CutoffPeriodic) == (0, 1, 2)
    assert force.getNonbondedMethod() == force.NoCutoff and not force.usesPeriodicBoundaryConditions()
    assert force.addParticle(3.0 * unit.angstrom, 0.5 * unit.kilocalorie_per_mole, -1, -1, 0.3, 0.3, 0.3, 1, 1, 1) == 0
    assert force.addParticle(0.3, 1.5, 0, -1, 5.0 * unit.angstrom, 0.3, 0.3, 1.0, 2.0, 2.0) == 1
    assert force.getNumParticles() == 2
    sigma, eps, xp, yp, sx, sy, sz, ex, ey, ez = force.getParticleParameters(0)
    assert sigma.unit == unit.nanometer and eps.unit == unit.kilojoule_per_mole and sx.unit == unit.nanometer
    assert sigma._value == pytest.approx(0.3, rel=1e-15) and eps._value == pytest.approx(0.5 * 4.184, rel=1e-15)
    assert (xp, yp, ex, ey, ez) == (-1, -1, 1.0, 1.0, 1.0)
    assert force.getParticleParameters(1)[4]._value == pytest.approx(0.5, rel=1e-15)
    force.setParticleParameters(1, 0.31, 1.6, 0, -1, 0.6, 0.3, 0.3, 1.0, 3.0, 3.0)
    got = force.getParticleParameters(1)
    assert [got[0]._value, got[1]._value, got[2], got[3], got[4]._value, got[9]] == [0.31, 1.6, 0, -1, 0.6, 3.0]
    assert force.addException(0, 1, 0.25, 0.4) == 0
    with pytest.raises(openmm.OpenMMException, match='GayBerneForce: There is already an exception for particles 0 and 1'):
        force.addException(1, 0, 0.3, 0.0)
    assert force.addException(1, 0, 0.3, 0.0, True) == 0 and force.getNumExceptions() == 1
    i, j, s, e = force.getExceptionParameters(0)
    assert (i, j, s._value, e._value) == (1, 0, 0.3, 0.0) and s.unit == unit.nanometer and e.unit == unit.kilojoule_per_mole
    force.setExceptionParameters(0, 0, 1, 2.8 * unit.angstrom, 0.9)
    assert force.getExceptionParameters(0)[2]._value == pytest.approx(0.28, rel=1e-15)
    force.setNonbondedMethod(force.CutoffPeriodic)
    assert force.usesPeriodicBoundaryConditions()
    with pytest.raises(openmm.OpenMMException, match='Illegal value for nonbonded method'):
        force.setNonbondedMethod(3)
    force.setCutoffDistance(12.0 * unit.angstrom)
    assert force.getCutoffDistance()._value == pytest.approx(1.2, rel=1e-15) and force.getCutoffDistance().unit == unit.nanometer
    assert force.getUseSwitchingFunction() is False
    force.setUseSwitchingFunction(True)
    force.setSwitchingDistance(1.0)
    assert force.getUseSwitchingFunction() is True and force.getSwitchingDistance()._value == 1.0
    force.setForceGroup(7)
    assert force.getForceGroup() == 7


# ------------------------------------------------------------------------------------ what reaches the library
def test_translation_compacts_the_interacting_particles(recorder):
    spec = small_spec()
    system = bare_system(7, box=None)
    force = force_of(spec)
    force.setForceGroup(4)
    system.addForce(force)
    context = context_of(system)
    made = recorder[-1].gaybernes[0]
    # 0, 3 (markers) and 6 (epsilon 0, only in an exception with epsilon 0) never enter the scan; 5 does, through its exception
    assert made['active'].tolist() == [1, 2, 4, 5]
    assert made['axes'].tolist() == [[0, -1], [-1, -1], [0, 3], [-1, -1]]
    assert made['par'].shape == (4, 8)
    assert made['par'][0].tolist() == [0.3, 1.0] + list(GC.UNIAXIAL) and made['par'][2].tolist() == [0.3, 1.5] + list(GC.BIAXIAL)
    # the exceptions over ACTIVE indices, every pair on both rows, columns ascending: (1, 5) -> rows 0 / 3, (4, 2) -> rows 2 / 1
    assert made['ex_ptr'].tolist() == [0, 1, 2, 3, 4]
    assert made['ex_col'].tolist() == [3, 2, 1, 0]
    assert made['ex_par'].tolist() == [[0.31, 0.7], [0.3, 0.0], [0.3, 0.0], [0.31, 0.7]]
    # who names a particle: 0 is the x-particle of rows 0 and 2 (entries 0 and 4), 3 the y-particle of row 2 (entry 5)
    assert made['rev_ptr'].tolist() == [0, 2, 2, 2, 3, 3, 3, 3]
    assert made['rev_src'].tolist() == [0, 4, 5]
    assert (made['rc'], made['rs'], made['periodic']) == (0.0, -1.0, False)
    entry = [e for e in context._engine.entries if e.force is force][0]
    assert entry.term_ids == [made['id']] and entry.gayberne == made['id'] and entry.group == 4
    assert entry.depends == set() and entry.update is None          # deriv(energy, p): no dependence on any parameter
    assert context._engine.free_space


def test_translation_of_the_cutoff_the_switch_and_the_box(recorder):
    spec = small_spec()
    for method, switch, want in ((1, None, (0.9, -1.0, False)), (1, 0.7, (0.9, 0.7, False)), (2, 0.0, (0.9, 0.0, True)), (0, 0.7, (0.0, -1.0, False))):
        system = bare_system(7, box=3.0 if method == 2 else None)
        force = force_of(dict(spec, method=method, cutoff=0.9, switch=switch))
        system.addForce(force)
        context = context_of(system)
        made = recorder[-1].gaybernes[0]
        assert (made['rc'], made['rs'], made['periodic']) == want
        assert context._engine.free_space == (method != 2)


def test_many_exceptions_on_one_row_stay_sorted(recorder):
    spec, _, ell = GC.RECORDED['exc72'](place=False)
    system = bare_system(len(spec['particles']), box=None)
    system.addForce(force_of(spec))
    context_of(system)
    made = recorder[-1].gaybernes[0]
    assert made['active'].tolist() == ell
    counts = np.diff(made['ex_ptr'])
    assert counts[0] == 70 and counts[1] == 2 and counts[2] == 1 and counts[71] == 1 and counts.sum() == 142
    assert made['ex_col'][:70].tolist() == list(range(1, 71))
    for row in range(72):
        cols = made['ex_col'][made['ex_ptr'][row]:made['ex_ptr'][row + 1]]
        assert (np.diff(cols) > 0).all() and row not in cols
    assert made['ex_par'][made['ex_ptr'][71]].tolist() == [0.33, 2.5] and made['ex_col'][made['ex_ptr'][71]] == 1
    # markers interleaved: no active index equals its particle index
    assert all(k != p for k, p in enumerate(made['active']))
    assert made['rev_src'].tolist() == list(range(0, 144, 2)) and made['rev_ptr'][-1] == 72


def test_update_parameters_in_context(recorder):
    spec = small_spec()
    system = bare_system(7, box=None)
    force = force_of(spec)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    force.setParticleParameters(1, 0.33, 1.25, 0, -1, 0.6, 0.3, 0.3, 1.0, 2.0, 2.0)
    force.setExceptionParameters(0, 5, 1, 0.29, 0.8)
    force.updateParametersInContext(context)
    calls = [c for c in rec.calls if c[0] == 'gayberne_set_params']
    assert len(calls) == 1 and calls[0][1] == rec.gaybernes[0]['id']
    assert calls[0][2][0].tolist() == [0.33, 1.25, 0.6, 0.3, 0.3, 1.0, 2.0, 2.0]
    assert calls[0][3].tolist() == [[0.29, 0.8], [0.3, 0.0], [0.3, 0.0], [0.29, 0.8]]
    # what changes the tables' layout is refused by name and reaches nothing
    for change, message in ((lambda: force.setParticleParameters(6, 0.3, 1.0, -1, -1, 0.3, 0.3, 0.3, 1, 1, 1), 'the set of interacting particles'),
                            (lambda: force.setParticleParameters(1, 0.33, 1.25, 3, -1, 0.6, 0.3, 0.3, 1.0, 2.0, 2.0), 'the x- or y-particle of an ellipsoid'),
                            (lambda: force.setExceptionParameters(1, 4, 5, 0.3, 0.0), 'the pairs that have an exception')):
        fresh = force_of(spec)
        force._particles, force._exceptions = fresh._particles, fresh._exceptions
        change()
        with pytest.raises(openmm.OpenMMException, match='updateParametersInContext: %s' % message):
            force.updateParametersInContext(context)
    assert len([c for c in rec.calls if c[0] == 'gayberne_set_params']) == 1


# ------------------------------------------------------------------------------------ what is refused
def refused(recorder, spec, n, message, box=3.0, error=openmm.OpenMMException):
    system = bare_system(n, box=box)
    system.addForce(force_of(spec))
    with pytest.raises(error, match=message):
        context_of(system)
    assert not recorder or recorder[-1].gaybernes == []


def test_shapes_and_axis_particles_are_refused_by_name(recorder):
    ok = (0.3, 1.0)
    refused(recorder, GC.spec_of([MARKER, ok + (-1, -1) + GC.UNIAXIAL]), 2, 'particle 1 has no x-particle, which only a sphere')
    refused(recorder, GC.spec_of([MARKER, ok + (-1, -1, 0.3, 0.3, 0.3, 1.0, 1.0, 2.0)]), 2, 'particle 1 has no x-particle, which only a sphere')
    refused(recorder, GC.spec_of([MARKER, ok + (0, -1) + GC.BIAXIAL]), 2, 'particle 1 has no y-particle, which only a uniaxial shape')
    refused(recorder, GC.spec_of([MARKER, ok + (0, -1, 0.5, 0.3, 0.3, 1.0, 2.0, 2.5)]), 2, 'particle 1 has no y-particle, which only a uniaxial shape')
    refused(recorder, GC.spec_of([MARKER, ok + (-1, 0) + GC.SPHERE]), 2, 'particle 1 has a y-particle and no x-particle')
    refused(recorder, GC.spec_of([MARKER, ok + (2, -1) + GC.UNIAXIAL]), 2, 'an axis particle of particle 1 is out of range')
    refused(recorder, GC.spec_of([MARKER, ok + (0, -2) + GC.UNIAXIAL]), 2, 'an axis particle of particle 1 is out of range')
    refused(recorder, GC.spec_of([MARKER, ok + (1, -1) + GC.UNIAXIAL]), 2, 'particle 1 is its own axis particle')
    refused(recorder, GC.spec_of([MARKER, MARKER, ok + (0, 2) + GC.BIAXIAL]), 3, 'particle 2 is its own axis particle')
    refused(recorder, GC.spec_of([MARKER, ok + (0, -1) + GC.UNIAXIAL]), 3, 'GayBerneForce: the force has 2 particles, the System 3')
    refused(recorder, GC.spec_of([MARKER, ok + (0, -1, 0.5, 0.0, 0.0, 1.0, 2.0, 2.0)]), 2, 'diameters and well-depth scales above zero')
    refused(recorder, GC.spec_of([MARKER, MARKER], exceptions=[(0, 2, 0.3, 1.0)]), 2, 'exception 0 names a particle that does not exist')


def test_cutoffs_and_switches_are_refused_by_name(recorder):
    parts = [MARKER, (0.3, 1.0, 0, -1) + GC.UNIAXIAL]
    refused(recorder, GC.spec_of(parts, method=1, cutoff=1.0, switch=1.0), 2, r'the switching distance 1 lies outside \[0, cutoff = 1\)', box=None,
            error=InputError)
    refused(recorder, GC.spec_of(parts, method=2, cutoff=1.0, switch=-0.1), 2, r'the switching distance -0.1 lies outside \[0, cutoff = 1\)',
            error=InputError)
    refused(recorder, GC.spec_of(parts, method=2, cutoff=1.6), 2, r'GayBerneForce: the cutoff 1.6 exceeds half the shortest box edge \(3\)',
            error=InputError)
    refused(recorder, GC.spec_of(parts, method=1, cutoff=0.0), 2, 'GayBerneForce: the cutoff distance must be above zero', box=None, error=InputError)
    refused(recorder, GC.spec_of(parts, method=2, cutoff=1.0), 2, 'a GayBerneForce that uses periodic boundary conditions', box=None, error=InputError)


def test_too_many_interacting_particles_are_refused(recorder):
    n = E.Engine.GAYBERNE_MAX + 1
    assert E.Engine.GAYBERNE_MAX == 32768
    spec = GC.spec_of([(0.3, 1.0, -1, -1) + GC.SPHERE] * n)
    refused(recorder, spec, n, 'GayBerneForce: 32769 particles with epsilon > 0 \\(limit 32768\\)', box=None, error=InputError)


def test_ranks_collective_variables_and_virials_are_refused(recorder):
    spec = GC.spec_of([MARKER, (0.3, 1.0, 0, -1) + GC.UNIAXIAL])

    def job(rank):
        system = bare_system(2)
        system.addForce(force_of(dict(spec, method=2)))
        with pytest.raises(InputError, match='a GayBerneForce runs on a single rank'):
            context_of(system)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
    assert 'GayBerneForce' not in E.Engine._CV_INNER_CLASSES
    system = bare_system(2)
    cv = openmm.CustomCVForce('gb')
    cv.addCollectiveVariable('gb', force_of(spec))
    system.addForce(cv)
    with pytest.raises(NotImplementedError, match=r'CustomCVForce over a GayBerneForce \(collective variable gb\)'):
        context_of(system)
    system = bare_system(2)
    system.addForce(force_of(spec))
    with pytest.raises(NotImplementedError, match='ComputingSystem / PressureComputer: the virial of a GayBerneForce is not supported'):
        atomsmm.ComputingSystem(system)


def test_the_entry_points_are_exported():
    for name in ('amm_gayberne_create', 'amm_gayberne_set_params', 'amm_gayberne_stats', 'amm_gayberne_release'):
        assert name in B.EXPORTS


# ------------------------------------------------------------------------------------ the checker against closed forms
def test_checker_in_the_lennard_jones_limit():
    sigma, eps = 0.34, 0.9
    spec = GC.spec_of([(sigma, eps, -1, -1, sigma, sigma, sigma, 1.0, 1.0, 1.0)] * 2)
    pos = np.array([[0.1, -0.2, 0.3], [0.35, 0.05, 0.45]])
    out = GC.evaluate(spec, pos)
    r = np.linalg.norm(pos[1] - pos[0])
    want = 4 * eps * ((sigma / r) ** 12 - (sigma / r) ** 6)
    slope = 4 * eps * (12 * sigma ** 12 / r ** 13 - 6 * sigma ** 6 / r ** 7)
    assert out['energy'] == pytest.approx(want, rel=1e-14)
    assert out['forces'][1] == pytest.approx(slope * (pos[1] - pos[0]) / r, rel=1e-13)
    assert out['forces'][0] == pytest.approx(-out['forces'][1], rel=1e-15)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_checker_for_two_aligned_ellipsoids(axis):
    """Identical, aligned, approached along axis k: sigma12 = s_k, chi = e_k, eta = (a b + c^2) / (2 c sqrt(a b))."""
    shape = GC.BIAXIAL
    # particles: x-marker, y-marker, ellipsoid, twice; the frames are the coordinate axes
    parts, pos = [], []
    step = np.eye(3)[axis] * (shape[axis] + 0.03)
    for k in range(2):
        base = 3 * k
        parts += [MARKER, MARKER, (0.3, 1.2, base, base + 1) + shape]
        centre = np.array([0.2, 0.1, -0.3]) + k * step
        pos += [centre - [0.1, 0, 0], centre - [0.05, 0.08, 0], centre]
    spec = GC.spec_of(parts)
    total, pairs = GC.energy(spec, np.array(pos))
    assert len(pairs) == 1
    t = pairs[0][2]
    a, b, c = (0.5 * s for s in shape[:3])
    assert float(t['sigma12']) == pytest.approx(shape[axis], rel=1e-14)
    assert float(t['chi']) == pytest.approx(shape[3 + axis], rel=1e-14)
    assert float(t['eta']) == pytest.approx((a * b + c * c) / (2 * c * math.sqrt(a * b)), rel=1e-14)
    rho = 0.3 / (0.03 + 0.3)
    assert float(total) == pytest.approx(4 * 1.2 * (rho ** 12 - rho ** 6) * float(t['eta']) * shape[3 + axis], rel=1e-13)


def rigid_image(pos, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return pos @ q.T + rng.normal(size=3)


def test_checker_is_invariant_under_rigid_motion_and_axis_flips():
    spec, pos, ell = GC.fluid(6, 41, biaxial_every=2)
    base, _ = GC.energy(spec, pos)
    moved, _ = GC.energy(spec, rigid_image(pos, 42))
    # (the rotated positions are rounded to fp64: 1e-16 of 1 nm against a potential that changes by 1e3 kJ/mol per nm)
    assert float(moved) == pytest.approx(float(base), rel=1e-12)
    for flips in ({ell[0]: (-1, 1)}, {ell[0]: (1, -1)}, {ell[2]: (-1, -1), ell[1]: (-1, 1)}):
        flipped, _ = GC.energy(spec, pos, flips)
        with mpmath.workdps(GC.DIGITS):
            assert abs(flipped - base) <= abs(base) * mpmath.mpf('1e-45')


def test_checker_inverse_and_determinant():
    rng = np.random.default_rng(5)
    with mpmath.workdps(GC.DIGITS):
        for _ in range(5):
            a = rng.normal(size=(3, 3))
            M = [[mpmath.mpf(float(v)) for v in row] for row in (a @ a.T + np.eye(3))]
            v = [mpmath.mpf(float(c)) for c in rng.normal(size=3)]
            q, det = GC.quad_inverse(M, v)
            inv = mpmath.matrix(M) ** -1
            want = sum(v[i] * inv[i, j] * v[j] for i in range(3) for j in range(3))
            assert abs(q - want) <= abs(want) * mpmath.mpf('1e-45')
            assert abs(det - mpmath.det(mpmath.matrix(M))) <= abs(det) * mpmath.mpf('1e-45')


def test_checker_forces_sum_to_zero_and_follow_a_coarse_difference():
    spec, pos, ell = GC.fluid(5, 51, biaxial_every=2)
    out = GC.evaluate(spec, pos)
    f = out['forces']
    total = np.abs(f).sum()
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0
    # every row is rounded to fp64 once: n rows of 2^-53 relative each, times the lever (below 2 nm) for the torque
    assert np.abs(f.sum(axis=0)).max() <= len(f) * 2.0 ** -53 * np.abs(f).max()
    assert np.abs(np.cross(pos, f).sum(axis=0)).max() <= len(f) * 2.0 ** -53 * np.abs(f).max() * 2.0
    # an independent look at the step: h = 2^-24 nm on the fp64 positions; truncation h^2 E''' / 6 with E''' below 1e7 kJ/mol/nm^3
    # at these contacts (rho^12 differentiated three times): 3.6e-15 * 1e7 / 6 ~ 6e-9, far inside 1e-6 of sum|F| ~ 1e3
    h = 2.0 ** -24
    worst = 0.0
    for p in (0, ell[0], ell[1], len(pos) - 1):
        for axis in range(3):
            e = []
            for sign in (1, -1):
                moved = pos.copy()
                moved[p, axis] += sign * h
                e.append(float(GC.energy(spec, moved)[0]))
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - f[p, axis]))
    print('checker forces against a coarse difference: worst %.3e, sum|F| = %.4g' % (worst, total))
    assert worst <= 1e-6 * total


def test_switch_and_cutoff_in_the_checker():
    parts = [(0.3, 1.0, -1, -1) + GC.SPHERE] * 2
    pos = np.array([[0.0, 0.0, 0.0], [0.45, 0.0, 0.0]])
    plain = GC.evaluate(GC.spec_of(parts, method=1, cutoff=0.5), pos)['energy']
    lj = 4 * ((0.3 / 0.45) ** 12 - (0.3 / 0.45) ** 6)
    assert plain == pytest.approx(lj, rel=1e-14)                               # no shift
    t = (0.45 - 0.4) / (0.5 - 0.4)
    switched = GC.evaluate(GC.spec_of(parts, method=1, cutoff=0.5, switch=0.4), pos)['energy']
    assert switched == pytest.approx(lj * (1 - 10 * t ** 3 + 15 * t ** 4 - 6 * t ** 5), rel=1e-13)
    beyond = GC.evaluate(GC.spec_of(parts, method=1, cutoff=0.45), pos)
    assert beyond['energy'] == 0.0 and not beyond['forces'].any() and beyond['n_pairs'] == 0
    # periodic: the pair across a face is the pair at the image's distance
    wrapped = GC.evaluate(GC.spec_of(parts, method=2, cutoff=0.5, box=(2.0, 2.0, 2.0)), pos + [[0.9, 0, 0], [0.9 - 2.0, 0, 0]])['energy']
    assert wrapped == pytest.approx(lj, rel=1e-13)


# ------------------------------------------------------------------------------------ the recorded answers are the checker's
@pytest.mark.parametrize('name', sorted(GC.RECORDED))
def test_recorded_cases_are_what_the_checker_says(name):
    spec, pos, ell, out = GC.recorded(name)
    assert out['forces'].shape == pos.shape == (len(spec['particles']), 3)
    assert out['min_ratio'] >= 0.75 and out['max_rho'] > 1.0
    rows = [0, ell[len(ell) // 2], len(pos) - 1]                        # a marker, an ellipsoid, the last particle
    again = GC.evaluate(spec, pos, rows=rows, totals=False)
    assert np.array_equal(again['forces'][rows], out['forces'][rows])
    if len(ell) <= 72:
        assert float(GC.energy(spec, pos)[0]) == out['energy']
