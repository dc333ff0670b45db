"""CPU tests of CMAPTorsionForce and RBTorsionForce: the reference the GPU tests compare the kernel with (tests/cmap_cases.py) is
pinned here against central differences, the host's map coefficients (tables.cmap_coefficients) against that reference, and the host
layer -- the object model, the <CMAPTorsionForce> and <RBTorsionForce> sections of a force-field file, what the engine hands to the
library and everything it refuses -- runs on the call recorder."""
import copy

import numpy as np
import pytest

import atomsmm_amd as atomsmm
import cmap_cases as C
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd import tables as T
from atomsmm_amd.openmm import app
from fake_backend import RecordingContext


class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.cmaps, self.terms = [], []

    def cmap_create(self, sizes, coeffs, map_of_term, idx, periodic=False):
        fid = self._new()
        self.cmaps.append(dict(id=fid, sizes=np.array(sizes), coeffs=np.array(coeffs), maps=np.array(map_of_term), idx=np.array(idx),
                               periodic=bool(periodic)))
        return fid

    def cmap_set_params(self, fid, coeffs, map_of_term, n_maps):
        self.calls.append(('cmap_set_params', fid, np.array(coeffs), np.array(map_of_term), n_maps))

    def term_expr_create(self, kind, code, consts, globals_, idx, params, periodic=False):
        fid = self._new()
        self.terms.append(dict(id=fid, kind=kind, code=list(code), consts=list(consts), globals=list(globals_), idx=np.array(idx),
                               params=np.array(params), periodic=bool(periodic)))
        return fid

    def term_expr_set_params(self, fid, params, n_terms):
        self.calls.append(('term_expr_set_params', fid, np.array(params), n_terms))


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(Recorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def bare_system(n=10, box=True):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(12.0)
    if box:
        system.setDefaultPeriodicBoxVectors((3.0, 0, 0), (0, 3.0, 0), (0, 0, 3.0))
    return system


def context_of(system):
    return openmm.Context(system, openmm.VerletIntegrator(0.001))


def asymmetric_map(size):
    """size * size distinct values, energy[i + size * j] = 1 + (i + size * j) / size^2: in [1, 2)."""
    return 1.0 + np.arange(size * size) / float(size * size)


def cmap_force(periodic=False):
    force = openmm.CMAPTorsionForce()
    force.addMap(4, asymmetric_map(4))
    force.addMap(3, 2.0 + asymmetric_map(3))
    force.addTorsion(0, 0, 1, 2, 3, 1, 2, 3, 4)
    force.addTorsion(1, 1, 2, 3, 4, 2, 3, 4, 5)
    force.addTorsion(0, 9, 8, 7, 6, 8, 7, 6, 5)
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


# ------------------------------------------------------------------------------------ the reference itself
def test_reference_forces_are_the_gradient_of_its_energy():
    pos, terms = C.backbone(9, seed=3)
    terms = np.concatenate([terms, [[1, 0, 1, 2, 3, 0, 1, 2, 3]]])           # one term that names the same torsion twice
    maps = [C.random_map(5, 11), C.random_map(24, 12)]
    out = C.evaluate(pos, maps, terms)
    h = 1e-6
    worst = 0.0
    for atom in range(9):
        for axis in range(3):
            e = []
            for sign in (1, -1):
                moved = pos.copy()
                moved[atom, axis] += sign * h
                e.append(C.evaluate(moved, maps, terms, want_forces=False)['energy'])
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - out['forces'][atom, axis]))
    scale = np.abs(out['forces']).max()
    # central difference: truncation h^2 E''' / 6 -- third derivatives of a 24 x 24 map with values of order 1 are of order
    # 1 / delta^3 = 56 per radian^3, times |grad phi|^3 ~ (1 / 0.1 nm)^3: 6e4, so 1e-12 * 6e4 / 6 = 1e-8 --, rounding eps |E| / h ~
    # 1e-16 * 20 / 1e-6 = 2e-9; the bound leaves a factor of some tens over both
    print('reference forces against central differences: worst %.3e, max|F| = %.4g' % (worst, scale))
    assert scale > 1.0 and worst <= 1e-6 * scale
    assert np.abs(out['forces'].sum(axis=0)).max() <= 1e-12 * scale * 3


def test_reference_spline_interpolates_and_is_periodic():
    size, energy = 5, asymmetric_map(5)
    spline = C.MapSpline(size, energy)
    delta = 2 * np.pi / size
    for i in range(size):
        for j in range(size):
            assert spline(i * delta, j * delta)[0] == pytest.approx(energy[i + size * j], rel=1e-14)
    a, b = spline(0.3, -1.1), spline(0.3 + 2 * np.pi, -1.1 + 4 * np.pi)
    assert a == pytest.approx(b, rel=1e-12)


def test_place_dihedral_places_the_angles():
    for phi, psi in ((0.3, -1.2), (2.5, 3.0), (-2.0, 0.0), (np.pi, 0.5), (0.0, 0.0)):
        x = C.place_dihedral(phi, psi) + 1.0
        got = (C.dihedral(x, [0, 1, 2, 3])[0], C.dihedral(x, [1, 2, 3, 4])[0])
        assert np.allclose(np.mod(np.subtract(got, (phi, psi)) + np.pi, 2 * np.pi) - np.pi, 0.0, atol=1e-14)


# ------------------------------------------------------------------------------------ tables.cmap_coefficients
@pytest.mark.parametrize('size', [2, 3, 5, 24])
def test_coefficients_against_the_reference(size):
    rng = np.random.default_rng(100 + size)
    energy = rng.uniform(1.0, 3.0, size * size)
    coef = T.cmap_coefficients(size, energy)
    assert coef.shape == (size * size, 16) and coef.flags['C_CONTIGUOUS']
    spline = C.MapSpline(size, energy)
    top = np.abs(energy).max()
    worst = [0.0, 0.0]
    for phi, psi in rng.uniform(-np.pi, np.pi, (200, 2)):
        e, dphi, dpsi = T.cmap_eval(coef, size, phi, psi)
        e_ref, dphi_ref, dpsi_ref = spline(phi, psi)
        worst[0] = max(worst[0], abs(e - e_ref))
        worst[1] = max(worst[1], abs(dphi - dphi_ref), abs(dpsi - dpsi_ref))
    print('size %d: worst |dE| = %.3e, worst derivative deviation %.3e (max|map| %.3g)' % (size, worst[0], worst[1], top))
    assert worst[0] <= 1e-12 * top
    # a derivative is a difference of map values over delta = 2 pi / size: its scale, and its rounding, is size / (2 pi) times the map's
    assert worst[1] <= 1e-12 * top * size
    # at every node the patch returns the map value itself
    delta = 2 * np.pi / size
    for i in range(size):
        for j in range(size):
            assert coef[i + size * j, 0] == energy[i + size * j]
            assert T.cmap_eval(coef, size, i * delta, j * delta)[0] == pytest.approx(energy[i + size * j], rel=1e-13)


def test_coefficients_take_the_first_angle_fastest():
    size = 5
    energy = asymmetric_map(size)
    coef = T.cmap_coefficients(size, energy)
    delta = 2 * np.pi / size
    # one step in phi moves by one entry, one step in psi by `size` entries
    assert T.cmap_eval(coef, size, 1 * delta, 0.0)[0] == pytest.approx(energy[1], rel=1e-13)
    assert T.cmap_eval(coef, size, 0.0, 1 * delta)[0] == pytest.approx(energy[size], rel=1e-13)
    assert T.cmap_eval(coef, size, 3 * delta, 2 * delta)[0] == pytest.approx(energy[3 + size * 2], rel=1e-13)
    # negative angles are the same points as their images in [0, 2 pi)
    assert T.cmap_eval(coef, size, -2 * delta, -1 * delta)[0] == pytest.approx(energy[3 + size * 4], rel=1e-13)
    # the angle that rounds to 2 pi exactly lands in cell 0 at its node, not past the map
    assert T.cmap_eval(coef, size, -1e-17, -1e-17)[0] == energy[0]
    with pytest.raises(ValueError, match='size of at least 2'):
        T.cmap_coefficients(1, [1.0])
    with pytest.raises(ValueError, match='needs 25 values'):
        T.cmap_coefficients(5, np.zeros(24))


def test_a_constant_map_has_no_slope():
    coef = T.cmap_coefficients(6, np.full(36, 2.5))
    assert np.array_equal(coef[:, 0], np.full(36, 2.5)) and np.abs(coef[:, 1:]).max() <= 1e-15


# ------------------------------------------------------------------------------------ the object model
def test_cmap_object_model():
    force = openmm.CMAPTorsionForce()
    assert force.getNumMaps() == 0 and force.getNumTorsions() == 0 and not force.usesPeriodicBoundaryConditions()
    assert force.addMap(4, asymmetric_map(4)) == 0
    assert force.addMap(2, [1.0, 2.0, 3.0, 4.0] * unit.kilocalorie_per_mole) == 1
    assert force.getNumMaps() == 2
    size, energy = force.getMapParameters(0)
    assert size == 4 and np.array_equal(energy.value_in_unit(unit.kilojoule_per_mole), asymmetric_map(4))
    size, energy = force.getMapParameters(1)
    assert size == 2 and energy._value == pytest.approx([4.184, 8.368, 12.552, 16.736], rel=1e-15)
    force.setMapParameters(1, 3, np.arange(9.0))
    assert force.getMapParameters(1)[0] == 3 and force.getMapParameters(1)[1]._value == list(np.arange(9.0))
    for call in (lambda: force.addMap(1, [1.0]), lambda: force.addMap(4, np.zeros(15)), lambda: force.setMapParameters(0, 1, [1.0]),
                 lambda: force.setMapParameters(0, 3, np.zeros(16))):
        with pytest.raises(openmm.OpenMMException):
            call()
    assert force.getNumMaps() == 2 and force.getMapParameters(0)[0] == 4            # (a refused call changes nothing)
    assert force.addTorsion(1, 0, 1, 2, 3, 1, 2, 3, 4) == 0
    assert force.addTorsion(0, 5, 6, 7, 8, 6, 7, 8, 9) == 1
    assert force.getNumTorsions() == 2 and force.getTorsionParameters(1) == [0, 5, 6, 7, 8, 6, 7, 8, 9]
    force.setTorsionParameters(0, 0, 9, 8, 7, 6, 8, 7, 6, 5)
    assert force.getTorsionParameters(0) == [0, 9, 8, 7, 6, 8, 7, 6, 5]
    force.setUsesPeriodicBoundaryConditions(True)
    assert force.usesPeriodicBoundaryConditions()
    force.setForceGroup(7)
    assert force.getForceGroup() == 7 and copy.deepcopy(force).getNumTorsions() == 2
    with pytest.raises(openmm.OpenMMException):
        force.setForceGroup(32)


def test_rb_object_model():
    force = openmm.RBTorsionForce()
    assert force.getNumTorsions() == 0 and not force.usesPeriodicBoundaryConditions()
    assert force.addTorsion(0, 1, 2, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0) == 0
    assert force.addTorsion(1, 2, 3, 4, *[1.0 * unit.kilocalorie_per_mole] * 6) == 1
    row = force.getTorsionParameters(0)
    assert row[:4] == [0, 1, 2, 3] and [c.value_in_unit(unit.kilojoule_per_mole) for c in row[4:]] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert [c._value for c in force.getTorsionParameters(1)[4:]] == pytest.approx([4.184] * 6, rel=1e-15)
    force.setTorsionParameters(1, 4, 3, 2, 1, 0.5, 0.0, 0.0, 0.0, 0.0, -0.5)
    assert force.getTorsionParameters(1)[:4] == [4, 3, 2, 1] and force.getTorsionParameters(1)[9]._value == -0.5
    force.setUsesPeriodicBoundaryConditions(True)
    force.setForceGroup(2)
    assert force.usesPeriodicBoundaryConditions() and force.getForceGroup() == 2 and force.getNumTorsions() == 2


def test_molecules_follow_both_classes():
    system = bare_system(12)
    cmap = openmm.CMAPTorsionForce()
    cmap.addMap(2, [1.0, 2.0, 3.0, 4.0])
    cmap.addTorsion(0, 0, 1, 2, 3, 1, 2, 3, 4)
    rb = openmm.RBTorsionForce()
    rb.addTorsion(6, 7, 8, 9, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    system.addForce(cmap)
    system.addForce(rb)
    assert openmm.molecules_of(system) == [[0, 1, 2, 3, 4], [5], [6, 7, 8, 9], [10], [11]]


# ------------------------------------------------------------------------------------ what the engine hands over
def test_cmap_translation_groups_and_update(recorder):
    system = bare_system()
    force = cmap_force(periodic=True)
    force.setForceGroup(3)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    (made,) = rec.cmaps
    assert made['sizes'].tolist() == [4, 3] and made['periodic'] and made['maps'].tolist() == [0, 1, 0]
    assert made['idx'].tolist() == [[0, 1, 2, 3, 1, 2, 3, 4], [1, 2, 3, 4, 2, 3, 4, 5], [9, 8, 7, 6, 8, 7, 6, 5]]
    expected = np.concatenate([T.cmap_coefficients(4, asymmetric_map(4)).reshape(-1), T.cmap_coefficients(3, 2.0 + asymmetric_map(3)).reshape(-1)])
    assert made['coeffs'].shape == ((16 + 9) * 16,) and np.array_equal(made['coeffs'], expected)
    (entry,) = [e for e in context._engine.entries if e.force is force]
    assert entry.cmap == made['id'] and entry.term_ids == [made['id']] and not entry.pair_ids and entry.bonded_id is None and entry.group == 3
    # getState(groups=...) reaches it as a member of its group
    context.setPositions(np.random.default_rng(0).uniform(0.5, 2.5, (10, 3)))
    context.getState(getForces=True, groups={3})
    assert [c for c in rec.calls if c[0] == 'force_eval'] == [('force_eval', made['id'], True)]
    context.getState(getForces=True, groups={0})
    assert [c for c in rec.calls if c[0] == 'force_eval'].count(('force_eval', made['id'], True)) == 1
    # updateParametersInContext: new map values and a changed map index follow
    force.setMapParameters(1, 3, 5.0 + asymmetric_map(3))
    force.setTorsionParameters(2, 1, 9, 8, 7, 6, 8, 7, 6, 5)
    force.updateParametersInContext(context)
    (call,) = [c for c in rec.calls if c[0] == 'cmap_set_params']
    assert call[1] == made['id'] and call[3].tolist() == [0, 1, 1] and call[4] == 2
    assert np.array_equal(call[2][:256], expected[:256]) and np.array_equal(call[2][256:], T.cmap_coefficients(3, 5.0 + asymmetric_map(3)).reshape(-1))


def test_cmap_update_refuses_changed_atoms_sizes_and_counts(recorder):
    def fresh():
        system = bare_system()
        force = cmap_force()
        system.addForce(force)
        return force, context_of(system)

    force, context = fresh()
    force.setTorsionParameters(0, 0, 0, 1, 2, 4, 1, 2, 3, 4)
    with pytest.raises(openmm.OpenMMException, match='the particles of a torsion have changed'):
        force.updateParametersInContext(context)
    force, context = fresh()
    force.addTorsion(0, 0, 1, 2, 3, 1, 2, 3, 4)
    with pytest.raises(openmm.OpenMMException, match='the number of torsions has changed'):
        force.updateParametersInContext(context)
    force, context = fresh()
    force.addMap(4, asymmetric_map(4))
    with pytest.raises(openmm.OpenMMException, match='the number of maps has changed'):
        force.updateParametersInContext(context)
    force, context = fresh()
    force.setMapParameters(1, 4, asymmetric_map(4))
    with pytest.raises(openmm.OpenMMException, match='the size of a map has changed'):
        force.updateParametersInContext(context)
    force, context = fresh()
    force.setTorsionParameters(1, 2, 1, 2, 3, 4, 2, 3, 4, 5)
    with pytest.raises(openmm.OpenMMException, match='a map index is out of range'):
        force.updateParametersInContext(context)
    assert not [c for c in recorder[-1].calls if c[0] == 'cmap_set_params']
    other = cmap_force()
    with pytest.raises(openmm.OpenMMException, match='does not belong to this Context'):
        other.updateParametersInContext(context)


def test_cmap_in_free_space_and_bad_indices(recorder):
    system = bare_system(box=False)
    system.addForce(cmap_force())
    context = context_of(system)
    assert context._engine.free_space and recorder[-1].box is None and len(recorder[-1].cmaps) == 1 and not recorder[-1].cmaps[0]['periodic']
    system = bare_system(box=False)
    system.addForce(cmap_force(periodic=True))
    with pytest.raises(atomsmm.InputError, match='with a CMAPTorsionForce that uses periodic boundary conditions'):
        context_of(system)
    system = bare_system(n=9)
    system.addForce(cmap_force())
    with pytest.raises(openmm.OpenMMException, match='CMAPTorsionForce: a particle index is out of range'):
        context_of(system)
    system = bare_system()
    force = cmap_force()
    force.addTorsion(2, 0, 1, 2, 3, 1, 2, 3, 4)
    system.addForce(force)
    with pytest.raises(openmm.OpenMMException, match='CMAPTorsionForce: a map index is out of range'):
        context_of(system)


def test_a_respa_group_with_cmap_takes_the_plain_path(recorder):
    """RespaPropagator([2, 1]) with harmonic bonds and the CMAP force in the inner group 0: the group holds the bond-list set and the
    CMAP force as members of their own, the latter a member the scheduler's fusion rules decline (csrc/run_ops.hip)."""
    system = bare_system()
    bonds = openmm.HarmonicBondForce()
    for k in range(9):
        bonds.addBond(k, k + 1, 0.15, 1000.0)
    system.addForce(bonds)
    system.addForce(cmap_force())
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(system, integrator)
    context.setPositions(C.chain(np.random.default_rng(4), 10, start=(1.5, 1.5, 1.5)))
    integrator.step(1)
    rec = recorder[-1]
    cid = rec.cmaps[0]['id']
    assert cid in rec.groups[0][1] and rec.bonded[-1]['id'] in rec.groups[0][1]
    assert any(op[0] == B.OP_EVAL and op[1] == 0 for ops, _ in rec.runs for op in ops)


# ------------------------------------------------------------------------------------ RB: the lowering
def test_rb_lowers_to_the_torsion_text(recorder):
    system = bare_system()
    force = openmm.RBTorsionForce()
    force.addTorsion(0, 1, 2, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
    force.addTorsion(4, 5, 6, 7, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
    force.setUsesPeriodicBoundaryConditions(True)
    force.setForceGroup(1)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    assert E.Engine.RB_TEXT == 'c0 + cp*(c1 + cp*(c2 + cp*(c3 + cp*(c4 + cp*c5)))); cp = -cos(theta)'
    (made,) = rec.terms
    assert made['kind'] == B.TERM_TORSION and made['periodic'] and made['idx'].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # parameter-major, in the order c0 .. c5
    assert made['params'].tolist() == [[1.0, 0.1], [2.0, 0.2], [3.0, 0.3], [4.0, 0.4], [5.0, 0.5], [6.0, 0.6]]
    # the same words as a CustomTorsionForce with that text
    twin = openmm.CustomTorsionForce(E.Engine.RB_TEXT)
    for k in range(6):
        twin.addPerTorsionParameter('c%d' % k)
    twin.addTorsion(0, 1, 2, 3, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    other = bare_system()
    other.addForce(twin)
    context_of(other)
    assert recorder[-1].terms[0]['code'] == made['code'] and recorder[-1].terms[0]['consts'] == made['consts']
    (entry,) = [e for e in context._engine.entries if e.force is force]
    assert entry.term_ids == [made['id']] and entry.term_expr and entry.group == 1
    # updateParametersInContext re-uploads the coefficients; changed atoms are refused
    force.setTorsionParameters(1, 4, 5, 6, 7, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0)
    force.updateParametersInContext(context)
    (call,) = [c for c in rec.calls if c[0] == 'term_expr_set_params']
    assert call[1] == made['id'] and call[2][:, 1].tolist() == [9.0, 8.0, 7.0, 6.0, 5.0, 4.0] and call[2][:, 0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    force.setTorsionParameters(1, 4, 5, 6, 8, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0)
    with pytest.raises(openmm.OpenMMException, match='the particles of the torsions have changed'):
        force.updateParametersInContext(context)


def test_rb_text_is_the_closed_form():
    """The lowered text, run by the host restatement of the interpreter's arithmetic, against sum c_n cos(psi)^n, psi = phi - pi."""
    from atomsmm_amd import expr as X
    c = [1.3, -2.1, 0.7, 3.3, -0.4, 1.9]
    for phi in (-3.0, -1.2, 0.0, 0.4, 2.9, np.pi):
        value = X.eval_global(E.Engine.RB_TEXT, dict(theta=phi, **{'c%d' % k: c[k] for k in range(6)}))
        assert value == pytest.approx(sum(c[n] * np.cos(phi - np.pi) ** n for n in range(6)), rel=1e-13)


# ------------------------------------------------------------------------------------ refusals, by name
def test_refusals_by_name(recorder):
    def job(rank):
        system = bare_system()
        system.addForce(cmap_force())
        with pytest.raises(NotImplementedError, match='CMAPTorsionForce runs on a single rank'):
            context_of(system)
        system = bare_system()
        rb = openmm.RBTorsionForce()
        rb.addTorsion(0, 1, 2, 3, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        system.addForce(rb)
        with pytest.raises(NotImplementedError, match='RBTorsionForce runs on a single rank'):
            context_of(system)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
    # as a collective variable
    system = bare_system()
    cv = openmm.CustomCVForce('0.5*k*(v - 2)^2')
    cv.addGlobalParameter('k', 10.0)
    cv.addCollectiveVariable('v', cmap_force())
    system.addForce(cv)
    with pytest.raises(NotImplementedError, match='CustomCVForce over a CMAPTorsionForce'):
        context_of(system)
    # RB in free space with the periodic flag
    system = bare_system(box=False)
    rb = openmm.RBTorsionForce()
    rb.addTorsion(0, 1, 2, 3, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    rb.setUsesPeriodicBoundaryConditions(True)
    system.addForce(rb)
    with pytest.raises(atomsmm.InputError, match='with a RBTorsionForce that uses periodic boundary conditions'):
        context_of(system)
    # a class that is still unknown stays refused

    class UnknownForce(openmm.Force):
        pass
    system = bare_system()
    system.addForce(UnknownForce())
    with pytest.raises(atomsmm.InputError, match='force type UnknownForce is not supported by the HIP path'):
        context_of(system)


def test_backend_exports_the_three_entry_points():
    for name in ('amm_cmap_create', 'amm_cmap_set_params', 'amm_cmap_release'):
        assert name in B.EXPORTS
    for name in ('cmap_create', 'cmap_set_params', 'cmap_release'):
        assert callable(getattr(B.HipContext, name))


# ------------------------------------------------------------------------------------ the force-field file
FIELD = """<ForceField>
 <AtomTypes>
  <Type name="tN" class="N" element="N" mass="14.0"/><Type name="tCA" class="CT" element="C" mass="12.0"/>
  <Type name="tC" class="C" element="C" mass="12.0"/><Type name="tO" class="O" element="O" mass="16.0"/>
  <Type name="tX" class="X" element="C" mass="12.0"/>
 </AtomTypes>
 <Residues>
  <Residue name="FWD"><Atom name="A1" type="tC"/><Atom name="A2" type="tN"/><Atom name="A3" type="tCA"/><Atom name="A4" type="tC"/><Atom name="A5" type="tN"/>
   <Bond from="0" to="1"/><Bond from="1" to="2"/><Bond from="2" to="3"/><Bond from="3" to="4"/></Residue>
  <Residue name="REV"><Atom name="B1" type="tN"/><Atom name="B2" type="tC"/><Atom name="B3" type="tCA"/><Atom name="B4" type="tN"/><Atom name="B5" type="tC"/>
   <Bond from="0" to="1"/><Bond from="1" to="2"/><Bond from="2" to="3"/><Bond from="3" to="4"/></Residue>
  <Residue name="OTH"><Atom name="D1" type="tX"/><Atom name="D2" type="tN"/><Atom name="D3" type="tCA"/><Atom name="D4" type="tC"/><Atom name="D5" type="tO"/>
   <Bond from="0" to="1"/><Bond from="1" to="2"/><Bond from="2" to="3"/><Bond from="3" to="4"/></Residue>
 </Residues>
 <CMAPTorsionForce>
  <Map>
   0 1 2 3
   4 5 6 7
   8 9 10 11
   12 13 14 15
  </Map>
  <Map> 1.5 2.5 3.5 4.5 </Map>
  <Torsion map="0" class1="C" class2="N" class3="CT" class4="C" class5="N"/>
  <Torsion map="1" type1="tX" type2="tN" type3="tCA" type4="tC" type5="tO"/>
 </CMAPTorsionForce>
 RB_SECTION
</ForceField>"""
RB_SECTION = """<RBTorsionForce>
  <Proper class1="C" class2="N" class3="CT" class4="C" c0="1.0" c1="2.0" c2="3.0" c3="4.0" c4="5.0" c5="6.0"/>
  <Proper type1="" type2="tCA" type3="tC" type4="" c0="0.5" c1="0" c2="0" c3="0" c4="0" c5="-0.5"/>
 </RBTorsionForce>"""


def chain_topology(residues):
    top = app.Topology()
    chain = top.addChain()
    for name, prefix in residues:
        res = top.addResidue(name, chain)
        atoms = [top.addAtom('%s%d' % (prefix, k), None, res) for k in range(1, 6)]
        for a, b in zip(atoms[:-1], atoms[1:]):
            top.addBond(a, b)
    return top


def test_forcefield_reads_the_cmap_section(tmp_path):
    (path := tmp_path / 'chain.xml').write_text(FIELD.replace('RB_SECTION', ''))
    field = app.ForceField(str(path))
    system = field.createSystem(chain_topology([('FWD', 'A'), ('REV', 'B'), ('OTH', 'D')]), removeCMMotion=False)
    (force,) = [f for f in system.getForces() if isinstance(f, openmm.CMAPTorsionForce)]
    assert force.getNumMaps() == 2
    # the file's values start at -180 degrees: both indices move by size // 2
    size, energy = force.getMapParameters(0)
    values = np.arange(16.0)
    assert size == 4 and energy._value == [values[(i + 2) % 4 + 4 * ((j + 2) % 4)] for j in range(4) for i in range(4)]
    assert energy._value[0] == 10.0 and energy._value[1] == 11.0 and energy._value[4] == 14.0 and energy._value[2 + 4 * 2] == 0.0
    size, energy = force.getMapParameters(1)
    assert size == 2 and energy._value == [4.5, 3.5, 2.5, 1.5]
    rows = sorted(force.getTorsionParameters(k) for k in range(force.getNumTorsions()))
    # FWD matches as written (classes), REV read from its other end, OTH by types; each chain once
    assert rows == [[0, 0, 1, 2, 3, 1, 2, 3, 4], [0, 9, 8, 7, 6, 8, 7, 6, 5], [1, 10, 11, 12, 13, 11, 12, 13, 14]]
    # a file without the section makes no such force
    (bare := tmp_path / 'bare.xml').write_text(FIELD.replace('RB_SECTION', '').split('<CMAPTorsionForce>')[0] + '</ForceField>')
    plain = app.ForceField(str(bare)).createSystem(chain_topology([('FWD', 'A')]))
    assert not any(isinstance(f, (openmm.CMAPTorsionForce, openmm.RBTorsionForce)) for f in plain.getForces())
    # a map that is no square, and a torsion that names a map the section does not have
    (bad := tmp_path / 'bad.xml').write_text(FIELD.replace('RB_SECTION', '').replace('1.5 2.5 3.5 4.5', '1.5 2.5 3.5'))
    with pytest.raises(ValueError, match='size\\*size values'):
        app.ForceField(str(bad))
    (bad2 := tmp_path / 'bad2.xml').write_text(FIELD.replace('RB_SECTION', '').replace('map="1"', 'map="2"'))
    with pytest.raises(ValueError, match='names map 2'):
        app.ForceField(str(bad2))


def test_forcefield_system_runs_on_the_recorder(tmp_path, recorder):
    (path := tmp_path / 'chain.xml').write_text(FIELD.replace('RB_SECTION', RB_SECTION))
    system = app.ForceField(str(path)).createSystem(chain_topology([('FWD', 'A'), ('OTH', 'D')]), removeCMMotion=False)
    context_of(system)
    rec = recorder[-1]
    assert rec.box is None and len(rec.cmaps) == 1 and rec.cmaps[0]['sizes'].tolist() == [4, 2] and rec.cmaps[0]['maps'].tolist() == [0, 1]
    assert len(rec.terms) == 1 and rec.terms[0]['kind'] == B.TERM_TORSION


def test_forcefield_reads_rb_propers_and_refuses_rb_impropers(tmp_path):
    (path := tmp_path / 'chain.xml').write_text(FIELD.replace('RB_SECTION', RB_SECTION))
    system = app.ForceField(str(path)).createSystem(chain_topology([('FWD', 'A')]), removeCMMotion=False)
    (force,) = [f for f in system.getForces() if isinstance(f, openmm.RBTorsionForce)]
    rows = sorted([r[:4] + [c._value for c in r[4:]] for r in (force.getTorsionParameters(k) for k in range(force.getNumTorsions()))])
    # C-N-CT-C over atoms 0..3 by classes (exact entries before wildcards); N-CT-C-N over atoms 1..4 by the wildcard entry
    assert rows == [[0, 1, 2, 3, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [1, 2, 3, 4, 0.5, 0.0, 0.0, 0.0, 0.0, -0.5]]
    improper = RB_SECTION.replace('</RBTorsionForce>', '<Improper class1="C" class2="N" class3="CT" class4="C" c0="1" c1="0" c2="0" c3="0" c4="0" c5="0"/></RBTorsionForce>')
    (bad := tmp_path / 'improper.xml').write_text(FIELD.replace('RB_SECTION', improper))
    with pytest.raises(NotImplementedError, match='<RBTorsionForce>: <Improper> entries are not supported'):
        app.ForceField(str(bad))
