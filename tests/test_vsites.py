"""CPU tests of virtual sites: the numpy restatement (tests/vsite_ref.py) against central differences and the conservation laws, the
System / Context object model with its validation, and app.ForceField on the TIP4P-Ew fixture (tests/golden/data/tip4pew.xml).
No GPU: a Context that must be refused is refused before the engine touches a device."""
import copy
import math
import os

import numpy as np
import pytest

import vsite_ref as VR
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.utils import InputError

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'data', 'tip4pew.xml')
R_OH, THETA, D_OM = 0.09572, math.radians(104.52), 0.0125
W_H = D_OM / (2.0 * R_OH * math.cos(0.5 * THETA))
W_O = 1.0 - 2.0 * W_H


def random_triangles(rng, count):
    """`count` triangles of parents (atoms 3t .. 3t + 2) with one site of each kind over every one (atoms 3 count + 3 t + kind)."""
    x = np.zeros((6 * count, 3))
    sites = []
    for t in range(count):
        o = rng.uniform(0, 3, 3)
        x[3 * t:3 * t + 3] = o + rng.normal(0, 0.1, (3, 3))
        w = rng.uniform(-0.5, 1.0, 3)
        sites.append((3 * count + 3 * t, VR.AVERAGE2, (3 * t + 1, 3 * t), (w[0], 1 - w[0])))
        sites.append((3 * count + 3 * t + 1, VR.AVERAGE3, (3 * t + 2, 3 * t, 3 * t + 1), (w[0], w[1], 1 - w[0] - w[1])))
        sites.append((3 * count + 3 * t + 2, VR.OUT_OF_PLANE, (3 * t, 3 * t + 1, 3 * t + 2), (w[1], w[2], 5.0 * w[0])))
    return x, VR.table(sites)


def test_spread_is_the_transposed_jacobian_of_place():
    """fp64, random triangles: spread(f) = J^T f with J from central differences of place (step 1e-6 nm), to 1e-8 relative."""
    rng = np.random.default_rng(11)
    count = 6
    x0, T = random_triangles(rng, count)
    x0 = VR.place(x0, *T)
    f = rng.normal(0, 300.0, x0.shape)
    got = VR.spread(x0, f, *T)
    site = T[0]
    want = np.array(f, copy=True)
    want[site] = 0.0
    h = 1e-6
    for p in range(3 * count):                   # every parent coordinate
        for k in range(3):
            xp, xm = x0.copy(), x0.copy()
            xp[p, k] += h
            xm[p, k] -= h
            dsdx = (VR.site_positions(xp, *T) - VR.site_positions(xm, *T)) / (2 * h)        # [ns][3]
            want[p, k] += np.sum(dsdx * f[site])
    scale = np.abs(want).max()
    print('max |spread - J^T f| / max|f| = %.2e' % (np.abs(got - want).max() / scale))
    assert np.abs(got - want).max() <= 1e-8 * scale
    assert np.all(got[site] == 0.0)


def test_spread_conserves_net_force_and_torque():
    rng = np.random.default_rng(12)
    x0, T = random_triangles(rng, 40)
    x0 = VR.place(x0, *T)
    f = rng.normal(0, 300.0, x0.shape)
    g = VR.spread(x0, f, *T)
    net = np.abs(f.sum(axis=0) - g.sum(axis=0)).max() / np.abs(f).sum()
    tq0, tq1 = np.cross(x0, f).sum(axis=0), np.cross(x0, g).sum(axis=0)
    torque = np.abs(tq0 - tq1).max() / np.abs(np.cross(x0, f)).sum()
    print('net force %.2e, net torque %.2e (relative)' % (net, torque))
    assert net <= 1e-13 and torque <= 1e-13


def test_place_kinds_by_hand():
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [9, 9, 9], [9, 9, 9], [9, 9, 9]])
    T = VR.table([(3, VR.AVERAGE2, (0, 1), (0.25, 0.75)), (4, VR.AVERAGE3, (0, 1, 2), (0.5, 0.25, 0.25)),
                  (5, VR.OUT_OF_PLANE, (0, 1, 2), (0.5, 0.5, 2.0))])
    out = VR.place(x, *T)
    assert np.array_equal(out[3], [0.75, 0, 0]) and np.array_equal(out[4], [0.25, 0.5, 0]) and np.array_equal(out[5], [0.5, 1.0, 4.0])
    assert np.array_equal(out[:3], x[:3])


# ------------------------------------------------------------------------------------------------ object model
def water4_system(n_waters=2, constraints=False):
    system = openmm.System()
    for w in range(n_waters):
        o = system.addParticle(15.99943)
        h1, h2 = system.addParticle(1.007947), system.addParticle(1.007947)
        m = system.addParticle(0.0)
        system.setVirtualSite(m, openmm.ThreeParticleAverageSite(o, h1, h2, W_O, W_H, W_H))
        if constraints:
            system.addConstraint(o, h1, R_OH)
            system.addConstraint(o, h2, R_OH)
    system.setDefaultPeriodicBoxVectors((3, 0, 0), (0, 3, 0), (0, 0, 3))
    nb = openmm.NonbondedForce()
    for i in range(system.getNumParticles()):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.CutoffPeriodic)
    system.addForce(nb)
    return system


def test_site_classes_and_system_api():
    two = openmm.TwoParticleAverageSite(3, 5, 0.25, 0.75)
    assert two.getNumParticles() == 2 and [two.getParticle(k) for k in range(2)] == [3, 5]
    assert [two.getWeight(k) for k in range(2)] == [0.25, 0.75]
    three = openmm.ThreeParticleAverageSite(1, 2, 4, 0.5, 0.3, 0.2)
    assert three.getNumParticles() == 3 and [three.getParticle(k) for k in range(3)] == [1, 2, 4]
    assert [three.getWeight(k) for k in range(3)] == [0.5, 0.3, 0.2]
    oop = openmm.OutOfPlaneSite(7, 8, 9, 0.1, 0.2, -0.3)
    assert oop.getNumParticles() == 3 and oop.getParticle(2) == 9
    assert (oop.getWeight12(), oop.getWeight13(), oop.getWeightCross()) == (0.1, 0.2, -0.3)
    assert all(isinstance(s, openmm.VirtualSite) for s in (two, three, oop))
    with pytest.raises(NotImplementedError, match='LocalCoordinatesSite'):
        openmm.LocalCoordinatesSite(0, 1, 2, (1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0))
    system = water4_system()
    assert [system.isVirtualSite(i) for i in range(8)] == [False, False, False, True] * 2
    site = system.getVirtualSite(7)
    assert [site.getParticle(k) for k in range(3)] == [4, 5, 6] and site.getWeight(0) == W_O
    with pytest.raises(openmm.OpenMMException):
        system.getVirtualSite(0)
    with pytest.raises(openmm.OpenMMException):
        system.setVirtualSite(8, two)
    clone = copy.deepcopy(system)
    other = openmm.System()
    other._copy_from(system)
    for s in (clone, other):
        assert s.isVirtualSite(3) and not s.isVirtualSite(2)
        assert s.getVirtualSite(3) is not system.getVirtualSite(3)
        assert s.getVirtualSite(3).getWeight(1) == W_H and s.getVirtualSite(7).getParticle(0) == 4


def test_molecules_join_a_site_to_its_parents():
    system = water4_system(constraints=True)
    assert openmm.molecules_of(system) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # a lone pair over three atoms that nothing else joins: the site alone makes them one molecule, as in OpenMM
    bare = openmm.System()
    for m in (12.0, 12.0, 12.0, 0.0, 12.0):
        bare.addParticle(m)
    bare.setVirtualSite(3, openmm.OutOfPlaneSite(0, 1, 2, 0.1, 0.1, 0.5))
    assert openmm.molecules_of(bare) == [[0, 1, 2, 3], [4]]


def refused(system, integrator=None):
    return openmm.Context(system, integrator or openmm.VerletIntegrator(0.001))


def test_validation_when_a_context_is_created():
    system = water4_system()
    system.setParticleMass(3, 1.0)
    with pytest.raises(openmm.OpenMMException, match='nonzero mass'):
        refused(system)
    system = water4_system()
    system.setVirtualSite(7, openmm.TwoParticleAverageSite(3, 4, 0.5, 0.5))          # parent 3 is a site
    with pytest.raises(openmm.OpenMMException, match='is a virtual site itself'):
        refused(system)
    system = water4_system()
    system.addConstraint(0, 3, 0.0125)
    with pytest.raises(openmm.OpenMMException, match='constraint cannot involve a virtual site'):
        refused(system)
    system = water4_system()
    massless = system.addParticle(0.0)
    system.getForce(0).addParticle(0.0, 0.3, 0.0)
    system.addConstraint(0, massless, 0.1)
    with pytest.raises(openmm.OpenMMException, match='constraint cannot involve a massless particle'):
        refused(system)
    system = water4_system()
    system.setVirtualSite(3, openmm.ThreeParticleAverageSite(0, 1, 8, W_O, W_H, W_H))
    with pytest.raises(openmm.OpenMMException, match='out of range'):
        refused(system)


def test_massless_systems_are_refused_by_name_where_nothing_skips_them():
    import atomsmm_amd as atomsmm
    system = water4_system()
    nhl = atomsmm.NHL_R_Integrator(1 * unit.femtoseconds, [1], 300 * unit.kelvin, 10 * unit.femtoseconds, 1 / unit.picoseconds)
    with pytest.raises(InputError, match='massless particles or virtual sites.*Nose-Hoover-Langevin'):
        refused(system, nhl)
    sinr = atomsmm.SIN_R_Integrator(1 * unit.femtoseconds, [1], 300 * unit.kelvin, 10 * unit.femtoseconds, 1 / unit.picoseconds)
    with pytest.raises(InputError, match='massless particles or virtual sites.*isokinetic'):
        refused(system, sinr)
    custom = openmm.CustomIntegrator(0.001)
    custom.addGlobalVariable('kT', 2.49)
    custom.addComputePerDof('x', 'x + c*tanh(1.0*v/c)*0.5*dt; c=sqrt(3.0*kT/m)')
    with pytest.raises(InputError, match='massless particles or virtual sites.*regulated'):
        refused(system, custom)
    custom = openmm.CustomIntegrator(0.001)
    custom.addGlobalVariable('g', 0.0)
    custom.addComputeGlobal('g', 'deriv(energy, lambda)')
    with pytest.raises(InputError, match=r'massless particles or virtual sites.*deriv\(energy'):
        refused(system, custom)
    inner = atomsmm.MultipleTimeScaleIntegrator(1 * unit.femtoseconds, [1])
    with pytest.raises(InputError, match='massless particles or virtual sites.*AdiabaticDynamicsIntegrator'):
        refused(system, atomsmm.AdiabaticDynamicsIntegrator(inner, 1, []))
    # a massless particle that is no site is refused the same way, and a System without either is not
    ghost = water4_system()
    ghost._vsites = {}
    with pytest.raises(InputError, match='massless particles or virtual sites.*Nose-Hoover-Langevin'):
        refused(ghost, atomsmm.NHL_R_Integrator(1 * unit.femtoseconds, [1], 300 * unit.kelvin, 10 * unit.femtoseconds, 1 / unit.picoseconds))
    # several ranks: their owner-integrating launches and exchanges neither place nor spread

    def job(rank):
        with pytest.raises(InputError, match='massless particles or virtual sites.*several ranks'):
            refused(water4_system())
        return True
    from atomsmm_amd import engine as E
    assert E.LocalWorld(2).run(job) == [True, True]
    computing = atomsmm.ComputingSystem(water4_system())
    with pytest.raises(InputError, match='massless particles or virtual sites.*ComputingSystem'):
        refused(computing, openmm.CustomIntegrator(0))


# ------------------------------------------------------------------------------------------------ app.ForceField
def two_water_topology():
    names = ['O', 'H1', 'H2', 'M'] * 2
    top = app.Topology.from_arrays(names, ['HOH'] * 8, residue_index=[0] * 4 + [1] * 4)
    top.setUnitCellDimensions((2.5, 2.5, 2.5))
    return top


def check_tip4pew(system, rigid=True):
    assert system.getNumParticles() == 8
    masses = [system.getParticleMass(i)._value for i in range(8)]
    assert masses == [15.99943, 1.007947, 1.007947, 0.0] * 2
    for w in range(2):
        b = 4 * w
        assert system.isVirtualSite(b + 3) and not any(system.isVirtualSite(b + k) for k in range(3))
        site = system.getVirtualSite(b + 3)
        assert isinstance(site, openmm.ThreeParticleAverageSite)
        assert [site.getParticle(k) for k in range(3)] == [b, b + 1, b + 2]
        # the weights from d_OM, not from the file's digits
        assert site.getWeight(0) == pytest.approx(W_O, rel=1e-12) and site.getWeight(1) == pytest.approx(W_H, rel=1e-12)
        assert site.getWeight(2) == pytest.approx(W_H, rel=1e-12)
    assert W_H == pytest.approx(0.1066767, rel=1e-6)
    angles = [f for f in system.getForces() if isinstance(f, openmm.HarmonicAngleForce)]
    bonds = [f for f in system.getForces() if isinstance(f, openmm.HarmonicBondForce)]
    if rigid:
        assert system.getNumConstraints() == 6
        cons = sorted((min(i, j), max(i, j), round(d, 9)) for i, j, d in system._constraints)
        r_hh = round(2 * R_OH * math.sin(0.5 * THETA), 9)
        assert cons == [(0, 1, R_OH), (0, 2, R_OH), (1, 2, r_hh), (4, 5, R_OH), (4, 6, R_OH), (5, 6, r_hh)]
        assert sum(f.getNumAngles() for f in angles) == 0 and sum(f.getNumBonds() for f in bonds) == 0
    else:
        assert system.getNumConstraints() == 0
        assert sum(f.getNumAngles() for f in angles) == 2 and sum(f.getNumBonds() for f in bonds) == 4
    nb = [f for f in system.getForces() if isinstance(f, openmm.NonbondedForce)][0]
    charges = [nb.getParticleParameters(i)[0]._value for i in range(8)]
    assert charges == [0.0, 0.52422, 0.52422, -1.04844] * 2
    assert nb.getParticleParameters(0)[1]._value == 0.316435 and nb.getParticleParameters(0)[2]._value == 0.680946
    # 6 excluded pairs per water (M-O is a 1-2 pair, M-H a 1-3 pair), none scaled
    assert nb.getNumExceptions() == 12
    pairs = set()
    for k in range(12):
        i, j, qq, _, eps = nb.getExceptionParameters(k)
        assert qq._value == 0.0 and eps._value == 0.0
        pairs.add((min(i, j), max(i, j)))
    assert pairs == {(b + i, b + j) for b in (0, 4) for i in range(4) for j in range(i + 1, 4)}


def test_forcefield_reads_the_tip4pew_fixture():
    ff = app.ForceField(FIXTURE)
    check_tip4pew(ff.createSystem(two_water_topology(), nonbondedMethod=app.PME, nonbondedCutoff=0.9 * unit.nanometers, rigidWater=True))
    check_tip4pew(ff.createSystem(two_water_topology(), nonbondedMethod=app.PME, nonbondedCutoff=0.9 * unit.nanometers, rigidWater=False),
                  rigid=False)
    # a rigid four-site water with HBonds on top: the same three constraints, no massless atom among them
    system = ff.createSystem(two_water_topology(), nonbondedMethod=app.CutoffPeriodic, constraints=app.HBonds, rigidWater=True)
    assert system.getNumConstraints() == 6
    openmm.check_virtual_sites(system)


def rewritten(tmp_path, old, new, name):
    text = open(FIXTURE).read()
    assert old in text
    path = tmp_path / name
    path.write_text(text.replace(old, new))
    return str(path)


SITE_BY_NAME = 'siteName="M" atomName1="O" atomName2="H1" atomName3="H2"'


def test_forcefield_reads_both_spellings(tmp_path):
    by_index = rewritten(tmp_path, SITE_BY_NAME, 'index="3" atom1="0" atom2="1" atom3="2"', 'by_index.xml')
    system = app.ForceField(by_index).createSystem(two_water_topology(), nonbondedMethod=app.PME, nonbondedCutoff=0.9 * unit.nanometers)
    check_tip4pew(system)


def test_forcefield_other_site_types(tmp_path):
    text = 'type="average3" ' + SITE_BY_NAME + ' weight1="0.7866465585518333" weight2="0.10667672072408337" weight3="0.10667672072408337"'
    two = rewritten(tmp_path, text, 'type="average2" siteName="M" atomName1="O" atomName2="H1" weight1="0.75" weight2="0.25"', 'two.xml')
    site = app.ForceField(two).createSystem(two_water_topology()).getVirtualSite(7)
    assert isinstance(site, openmm.TwoParticleAverageSite) and [site.getParticle(k) for k in range(2)] == [4, 5]
    assert [site.getWeight(k) for k in range(2)] == [0.75, 0.25]
    oop = rewritten(tmp_path, text, 'type="outOfPlane" index="3" atom1="0" atom2="1" atom3="2" weight12="0.1" weight13="0.2" weightCross="-0.3"',
                    'oop.xml')
    site = app.ForceField(oop).createSystem(two_water_topology()).getVirtualSite(3)
    assert isinstance(site, openmm.OutOfPlaneSite) and [site.getParticle(k) for k in range(3)] == [0, 1, 2]
    assert (site.getWeight12(), site.getWeight13(), site.getWeightCross()) == (0.1, 0.2, -0.3)


def test_forcefield_refuses_what_it_does_not_read(tmp_path):
    with pytest.raises(NotImplementedError, match='localCoords'):
        app.ForceField(rewritten(tmp_path, 'type="average3"', 'type="localCoords"', 'local.xml'))
    with pytest.raises(NotImplementedError, match='excludeWith'):
        app.ForceField(rewritten(tmp_path, 'siteName="M"', 'siteName="M" excludeWith="O"', 'exclude.xml'))
