"""CPU tests of RMSDForce: the object model, what the engine hands to the library and what it refuses -- on the call recorder -- and
the checker the GPU tests compare the kernels with (tests/rmsd_cases.py) against itself: its forces against central differences of
its own energy, its proper-rotation answer for a mirror image against numpy's SVD, and the sums of its forces and torques."""
import numpy as np
import pytest

import atomsmm_amd as atomsmm
import rmsd_cases as RC
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from fake_backend import RecordingContext


class Recorder(RecordingContext):
    def __init__(self, *a, **k):
        RecordingContext.__init__(self, *a, **k)
        self.rmsds, self.cvs = [], []

    def rmsd_create(self, particles, reference):
        fid = self._new()
        self.rmsds.append(dict(id=fid, particles=np.array(particles), reference=np.array(reference)))
        return fid

    def rmsd_set_reference(self, fid, particles, reference):
        self.calls.append(('rmsd_set_reference', fid, np.array(particles), np.array(reference)))

    def rmsd_release(self, fid):
        self.calls.append(('rmsd_release', fid))

    def cv_create(self, inner_ids, n_deriv, code, consts, globals_):
        fid = self._new()
        self.cvs.append(dict(id=fid, inner=list(inner_ids), n_deriv=n_deriv))
        return fid


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


REFERENCE = RC.blob(10, seed=1)


# ------------------------------------------------------------------------------------ the object model
def test_api_round_trips():
    force = openmm.RMSDForce(REFERENCE)
    assert force.getParticles() == []
    assert force.usesPeriodicBoundaryConditions() is False
    got = force.getReferencePositions()
    assert got.unit == unit.nanometer
    assert np.array_equal(np.array(got._value), REFERENCE)
    assert isinstance(got._value[0], openmm.Vec3)
    # with units: angstroms come back as nanometres
    force.setReferencePositions((10.0 * REFERENCE) * unit.angstrom)
    assert np.allclose(np.array(force.getReferencePositions()._value), REFERENCE, rtol=1e-15, atol=0)
    force.setReferencePositions([openmm.Vec3(*row) for row in REFERENCE] * unit.nanometer)
    assert np.array_equal(np.array(force.getReferencePositions()._value), REFERENCE)
    force.setParticles([7, 2, 5])
    assert force.getParticles() == [7, 2, 5]
    assert openmm.RMSDForce(REFERENCE, [3, 1]).getParticles() == [3, 1]
    force.setForceGroup(9)
    assert force.getForceGroup() == 9
    with pytest.raises(openmm.OpenMMException, match='Force group must be between 0 and 31'):
        force.setForceGroup(32)
    with pytest.raises(openmm.OpenMMException, match='one \\(x, y, z\\) per particle'):
        openmm.RMSDForce(np.zeros((4, 2)))


# ------------------------------------------------------------------------------------ what reaches the library
def test_translation_hands_over_the_listed_particles_and_their_rows(recorder):
    system = bare_system()
    force = openmm.RMSDForce(REFERENCE, [7, 2, 5])
    force.setForceGroup(3)
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    assert len(rec.rmsds) == 1
    made = rec.rmsds[0]
    assert made['particles'].tolist() == [7, 2, 5]
    assert np.array_equal(made['reference'], REFERENCE[[7, 2, 5]])
    entry = [e for e in context._engine.entries if e.force is force][0]
    assert entry.term_ids == [made['id']] and entry.rmsd == made['id'] and entry.group == 3
    assert entry.depends == set() and entry.update is None          # deriv(energy, p): no dependence on any parameter


def test_an_empty_list_means_all_particles(recorder):
    system = bare_system()
    system.addForce(openmm.RMSDForce(REFERENCE))
    context_of(system)
    made = recorder[-1].rmsds[0]
    assert made['particles'].tolist() == list(range(10))
    assert np.array_equal(made['reference'], REFERENCE)


def test_update_parameters_in_context_sets_the_reference_again(recorder):
    system = bare_system()
    force = openmm.RMSDForce(REFERENCE, [0, 1, 2, 3])
    system.addForce(force)
    context = context_of(system)
    rec = recorder[-1]
    fresh = RC.blob(10, seed=2)
    force.setReferencePositions(fresh)
    force.setParticles([9, 4, 6])                                     # (their number may change)
    force.updateParametersInContext(context)
    calls = [c for c in rec.calls if c[0] == 'rmsd_set_reference']
    assert len(calls) == 1
    _, fid, particles, reference = calls[0]
    assert fid == rec.rmsds[0]['id'] and particles.tolist() == [9, 4, 6]
    assert np.array_equal(reference, fresh[[9, 4, 6]])
    # a change the engine refuses reaches nothing
    force.setParticles([9, 9])
    with pytest.raises(openmm.OpenMMException, match='RMSDForce: a particle is listed twice'):
        force.updateParametersInContext(context)
    assert len([c for c in rec.calls if c[0] == 'rmsd_set_reference']) == 1


def test_as_a_collective_variable(recorder):
    assert 'RMSDForce' in E.Engine._CV_INNER_CLASSES
    system = bare_system()
    inner = openmm.RMSDForce(REFERENCE, [1, 2, 3, 4])
    cv = openmm.CustomCVForce('0.5*k*rmsd^2')
    cv.addGlobalParameter('k', 100.0)
    cv.addCollectiveVariable('rmsd', inner)
    system.addForce(cv)
    context_of(system)
    rec = recorder[-1]
    assert len(rec.rmsds) == 1 and len(rec.cvs) == 1
    assert rec.cvs[0]['inner'] == [rec.rmsds[0]['id']]
    assert rec.rmsds[0]['particles'].tolist() == [1, 2, 3, 4]
    # the inner force is a member of no group
    assert all(rec.rmsds[0]['id'] not in members for _slot, members in rec.groups.values())


# ------------------------------------------------------------------------------------ what is refused
def test_the_three_exceptions(recorder):
    for force, message in ((openmm.RMSDForce(REFERENCE[:9]), 'RMSDForce: 9 reference positions, the System has 10 particles'),
                           (openmm.RMSDForce(REFERENCE, [0, 10]), 'RMSDForce: a particle index is out of range'),
                           (openmm.RMSDForce(REFERENCE, [0, -1]), 'RMSDForce: a particle index is out of range'),
                           (openmm.RMSDForce(REFERENCE, [4, 2, 4]), 'RMSDForce: a particle is listed twice')):
        system = bare_system()
        system.addForce(force)
        with pytest.raises(openmm.OpenMMException, match=message):
            context_of(system)
        assert recorder[-1].rmsds == []


def test_several_ranks_and_the_virial_computers_are_refused(recorder):
    def job(rank):
        system = bare_system()
        system.addForce(openmm.RMSDForce(REFERENCE))
        with pytest.raises(NotImplementedError, match='RMSDForce runs on a single rank'):
            context_of(system)
        return True
    assert E.LocalWorld(2).run(job) == [True, True]
    system = bare_system()
    system.addForce(openmm.RMSDForce(REFERENCE))
    with pytest.raises(NotImplementedError, match='ComputingSystem / PressureComputer: the virial of an RMSDForce is not supported'):
        atomsmm.ComputingSystem(system)


def test_the_entry_points_are_exported():
    for name in ('amm_rmsd_create', 'amm_rmsd_set_reference', 'amm_rmsd_release'):
        assert name in B.EXPORTS


# ------------------------------------------------------------------------------------ the checker against itself
def test_checker_forces_are_the_gradient_of_its_energy():
    """N = 5, central differences with the step 2^-20 nm (exact in binary): the truncation is h^2 E''' / 6 with E''' of order
    1 / rmsd^2 ~ 1e2 per nm^2, 1e-12 * 1e2 / 6 ~ 2e-11, and the rounding of a 50-digit energy is nothing: within 1e-9 absolute."""
    ref = RC.blob(5, seed=11)
    pos = RC.displaced(ref, 12, 0.05)
    out = RC.evaluate(pos, ref)
    h = 2.0 ** -20
    worst = 0.0
    for atom in range(5):
        for axis in range(3):
            e = []
            for sign in (1, -1):
                moved = pos.copy()
                moved[atom, axis] += sign * h
                e.append(RC.evaluate(moved, ref, want_forces=False)['energy'])
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - out['forces'][atom, axis]))
    print('checker forces against central differences: worst %.3e, max|F| = %.4g' % (worst, np.abs(out['forces']).max()))
    assert np.abs(out['forces']).max() > 0.05
    assert worst <= 1e-9


def test_checker_counts_proper_rotations_only():
    ref, pos = RC.mirror_case(65, seed=5)
    out = RC.evaluate(pos, ref)
    kabsch = RC.kabsch_rmsd(pos, ref)
    print('mirror image: checker %.15g, SVD with the determinant correction %.15g' % (out['energy'], kabsch))
    # the SVD form is the eigenvalue-difference formula in fp64: eps * sum |y'|^2 / (N rmsd^2) ~ 1e-16 * 1.5 / 0.44 relative
    assert out['energy'] == pytest.approx(kabsch, rel=1e-13)
    assert out['energy'] > 0.5                                        # an improper fit would leave the noise: 0.02 * sqrt(3)
    # a subset in shuffled order is the same as the subset's own problem
    ref = RC.blob(30, seed=6)
    pos = RC.displaced(ref, 7, 0.05)
    sel = [17, 3, 22, 8, 11]
    sub = RC.evaluate(pos, ref, sel)
    own = RC.evaluate(pos[sel], ref[sel])
    assert sub['energy'] == own['energy'] and np.array_equal(sub['forces'][sel], own['forces'])
    assert not sub['forces'][[i for i in range(30) if i not in sel]].any()


def test_checker_forces_and_torques_sum_to_zero():
    ref = RC.blob(65, seed=21)
    pos = RC.displaced(ref, 22, 0.05)
    out = RC.evaluate(pos, ref)
    f = out['forces']
    top = np.abs(f).max()
    # 65 rows rounded to fp64 each: 65 * 2^-53 * max|F| for the force, times the lever (below 4 nm) for the torque
    assert np.abs(f.sum(axis=0)).max() <= 65 * 2.0 ** -53 * top
    assert np.abs(np.cross(pos - pos.mean(axis=0), f).sum(axis=0)).max() <= 65 * 2.0 ** -53 * top * 4.0
    # the rigid image itself: the defined zero
    still = RC.evaluate(RC.rigid_image(ref, 23), ref)
    assert still['energy'] == 0.0 and not still['forces'].any()
    # one particle: always zero
    one = RC.evaluate(pos[:1], ref[:1])
    assert one['energy'] == 0.0 and not one['forces'].any()
