"""CPU tests of the generalized-Born force (GBSAOBCForce): the fp64 restatement of the definition that the GPU tests compare the
kernels with (tests/gb_cases.py) is pinned here, and the host layer -- the object model, the <GBSAOBCForce> section of a force-field
file, what the engine hands to the library and everything it refuses -- runs on the call recorder."""
import copy
import io
import os

import numpy as np
import pytest

import atomsmm_amd as atomsmm
from atomsmm_amd import backend as B
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.testing import system_from_arrays
from conftest import GOLDEN
from fake_backend import RecordingContext
import gb_cases as G

REL = 1e-11


class GbRecorder(RecordingContext):
    def gb_create(self, q, radius, scale, eps_in=1.0, eps_out=78.3, sa_energy=2.25936, rc=0.0):
        fid = self._new()
        self.gbs = getattr(self, 'gbs', [])
        self.gbs.append(dict(id=fid, q=np.array(q), radius=np.array(radius), scale=np.array(scale), eps_in=eps_in, eps_out=eps_out,
                             sa_energy=sa_energy, rc=rc))
        return fid

    def gb_set_params(self, fid, q, radius, scale, eps_in=1.0, eps_out=78.3, sa_energy=2.25936, rc=0.0):
        self.calls.append(('gb_set_params', fid, np.array(q), np.array(radius), np.array(scale), eps_in, eps_out, sa_energy, rc))


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(GbRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


@pytest.fixture(scope='module')
def cases(heaq, spcfw):
    return {'N5': G.n5(), 'S33': G.with_radii(G.s33(heaq)), 'D1527': G.with_radii(G.d1527(spcfw))}


def add_gb(system, case, method=None, cutoff=1.0):
    gb = openmm.GBSAOBCForce()
    R, S = G.radii_by_mass(case['mass'])
    for q, r, s in zip(case['charge'], R, S):
        gb.addParticle(float(q), float(r), float(s))
    if method is not None:
        gb.setNonbondedMethod(method)
    gb.setCutoffDistance(cutoff)
    system.addForce(gb)
    return gb


# ------------------------------------------------------------------------------------ the restatement itself
def test_one_ion_has_the_closed_form():
    ion = dict(positions=np.zeros((1, 3)), charge=np.array([0.5]), radius=np.array([0.15]), scale=np.array([1.0]))
    out = G.evaluate(ion)
    closed = -0.5 * G.KC * (1 - 1 / 78.3) * 0.25 / 0.141 + 4 * np.pi * 2.25936 * 0.29 ** 2 * (0.15 / 0.141) ** 6
    assert out['energy'] == pytest.approx(-118.1355016683639, rel=REL)
    assert out['energy'] == pytest.approx(closed, rel=1e-14)
    assert out['born'][0] == pytest.approx(0.141, rel=1e-15) and not out['forces'].any()


PINNED = {('N5', None): (-410.46914881855025, 13.276715574567785), ('N5', 1.0): (-410.57952772010395, None),
          ('S33', None): (-102.628491444051, 21.4070825558199), ('S33', 1.0): (-101.57086606793, None),
          ('D1527', None): (-5752.81374148784, 455.713610231501), ('D1527', 1.0): (-10994.2233337441, 511.963084886504)}


@pytest.mark.parametrize('name,rc', sorted(PINNED, key=str))
def test_pinned_energies(cases, name, rc):
    out = G.evaluate(cases[name], rc, want_forces=False)
    e_pol, e_sa = PINNED[(name, rc)]
    assert out['e_pol'] == pytest.approx(e_pol, rel=REL)
    if e_sa is not None:
        assert out['e_sa'] == pytest.approx(e_sa, rel=REL)
    assert out['energy'] == out['e_pol'] + out['e_sa']


def test_n5_takes_every_branch_of_h():
    """The case is what its description says: checked on the geometry, not on the energies."""
    c = G.n5()
    rho = c['radius'] - G.OFFSET
    s = c['scale'] * rho
    r = np.linalg.norm(c['positions'][:, None] - c['positions'][None], axis=-1)
    assert rho[1] < s[0] - r[1, 0]                                   # atom 1 lies inside atom 0's scaled sphere
    assert not rho[0] < r[0, 1] + s[1]                               # the pair (0 <- 1) does not count
    for i, j in ((0, 2), (2, 0), (2, 3), (3, 2)):
        assert rho[i] < r[i, j] + s[j]                               # these count ...
    assert rho[0] > abs(r[0, 2] - s[2]) and rho[2] > abs(r[2, 3] - s[3])      # ... and the max picks rho
    assert rho[3] < abs(r[3, 4] - s[4])                              # and here |r - s|
    assert (r[4, :4] > 1.0).all() and (r[:4, :4] < 1.0).all()        # atom 4 alone lies outside a 1.0 nm cutoff


@pytest.mark.parametrize('name', ['N5', 'S33'])
@pytest.mark.parametrize('rc', [None, 1.0])
def test_the_blocked_evaluation_is_the_direct_one(cases, name, rc, monkeypatch):
    monkeypatch.setattr(G, 'ROWS', 7)              # several uneven blocks at 33 atoms
    blocked, direct = G.evaluate(cases[name], rc), G.evaluate_direct(cases[name], rc)
    assert blocked['energy'] == pytest.approx(direct['energy'], rel=1e-14)
    assert np.allclose(blocked['born'], direct['born'], rtol=1e-15, atol=0)
    assert np.abs(blocked['forces'] - direct['forces']).max() <= 1e-12 * np.abs(direct['forces']).max()


@pytest.mark.parametrize('name', ['N5', 'S33', 'D1527'])
@pytest.mark.parametrize('rc', [None, 1.0])
def test_autograd_forces_sum_to_zero(cases, name, rc):
    f = G.evaluate(cases[name], rc)['forces']
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).max() * np.sqrt(len(f))


@pytest.mark.parametrize('name,atom,axis', [('N5', 1, 0), ('N5', 2, 1), ('S33', 17, 2)])
def test_autograd_forces_agree_with_a_central_difference(cases, name, atom, axis):
    c = cases[name]
    f = G.evaluate(c)['forces'][atom, axis]
    h = 1e-5
    e = []
    for sign in (1, -1):
        moved = dict(c, positions=c['positions'].copy())
        moved['positions'][atom, axis] += sign * h
        e.append(G.evaluate(moved, want_forces=False)['energy'])
    # central difference: truncation h^2 E'''/6, rounding eps |E| / h ~ 1e-16 * 400 / 1e-5 = 4e-9
    assert -(e[0] - e[1]) / (2 * h) == pytest.approx(f, rel=1e-6, abs=1e-6)


def test_radii_by_mass():
    R, S = G.radii_by_mass([1.008, 12.01, 14.01, 16.0, 35.45])
    assert R.tolist() == [0.12, 0.17, 0.155, 0.15, 0.15] and S.tolist() == [0.85, 0.72, 0.79, 0.85, 0.85]


def test_d4608_is_three_boxes_in_a_row(spcfw):
    c = G.d4608(spcfw)
    assert len(c['positions']) == 4608 == 18 * 256
    assert np.array_equal(c['positions'][1536:3072], spcfw['positions'] + [spcfw['box'][0], 0, 0])
    assert np.array_equal(c['positions'][3072:], spcfw['positions'] + [2 * spcfw['box'][0], 0, 0])
    assert np.array_equal(c['charge'][3072:], spcfw['charge']) and np.array_equal(c['radius'][:3], [0.12, 0.15, 0.12])


# ------------------------------------------------------------------------------------ the object model
def test_object_model():
    gb = openmm.GBSAOBCForce()
    assert (gb.NoCutoff, gb.CutoffNonPeriodic, gb.CutoffPeriodic) == (0, 1, 2)
    assert gb.getSolventDielectric() == 78.3 and gb.getSoluteDielectric() == 1.0
    assert gb.getSurfaceAreaEnergy().value_in_unit(unit.kilojoule_per_mole / unit.nanometer ** 2) == 2.25936
    assert gb.getNonbondedMethod() == gb.NoCutoff and not gb.usesPeriodicBoundaryConditions()
    assert gb.addParticle(0.5 * unit.elementary_charge, 1.5 * unit.angstroms, 0.8) == 0
    assert gb.addParticle(-0.5, 0.17, 0.72) == 1
    assert gb.getNumParticles() == 2
    q, r, s = gb.getParticleParameters(0)
    assert q.value_in_unit(unit.elementary_charge) == 0.5 and r.value_in_unit(unit.nanometer) == pytest.approx(0.15, rel=1e-15) and s == 0.8
    gb.setParticleParameters(1, 0.25, 2.0 * unit.angstroms, 0.9)
    q, r, s = gb.getParticleParameters(1)
    assert (q._value, s) == (0.25, 0.9) and r._value == pytest.approx(0.2, rel=1e-15)
    gb.setSolventDielectric(80.0)
    gb.setSoluteDielectric(2.0)
    assert (gb.getSolventDielectric(), gb.getSoluteDielectric()) == (80.0, 2.0)
    gb.setSurfaceAreaEnergy(3.0 * unit.kilojoule_per_mole / unit.nanometer ** 2)
    assert gb.getSurfaceAreaEnergy()._value == 3.0
    gb.setNonbondedMethod(gb.CutoffNonPeriodic)
    gb.setCutoffDistance(12 * unit.angstroms)
    assert gb.getNonbondedMethod() == 1 and gb.getCutoffDistance().value_in_unit(unit.nanometer) == pytest.approx(1.2)
    assert not gb.usesPeriodicBoundaryConditions()
    gb.setNonbondedMethod(gb.CutoffPeriodic)
    assert gb.usesPeriodicBoundaryConditions()
    gb.setForceGroup(3)
    assert gb.getForceGroup() == 3 and copy.deepcopy(gb).getNumParticles() == 2


# ------------------------------------------------------------------------------------ the force-field file
def heaq_solute_topology():
    with open(os.path.join(GOLDEN, 'data', 'hydroxyethylaminoanthraquinone-in-water.pdb')) as fh:
        lines = [line for line in fh if line[:6] != 'CRYST1']
    atoms = [line for line in lines if line[:6] in ('ATOM  ', 'HETATM')][:33]
    return app.PDBFile(io.StringIO(''.join(atoms + [line for line in lines if line[:6] == 'CONECT'] + ['END\n'])))


def heaq_forcefield():
    return app.ForceField(os.path.join(GOLDEN, 'data', 'hydroxyethylaminoanthraquinone-in-water.xml'),
                          os.path.join(GOLDEN, 'data', 'gbsa-obc-heaq.xml'))


def test_forcefield_reads_the_gbsa_section(heaq):
    pdb = heaq_solute_topology()
    assert pdb.topology.getNumAtoms() == 33 and pdb.topology.getPeriodicBoxVectors() is None
    system = heaq_forcefield().createSystem(pdb.topology, rigidWater=False, removeCMMotion=False)
    (gb,) = [f for f in system.getForces() if isinstance(f, openmm.GBSAOBCForce)]
    case = G.with_radii(G.s33(heaq))
    assert gb.getNumParticles() == 33 and gb.getNonbondedMethod() == gb.NoCutoff
    par = np.array([[q._value, r._value, s] for q, r, s in (gb.getParticleParameters(k) for k in range(33))])
    # charges from the residue template (UseAttributeFromResidue), radii and scales by type or class: the mass table of gb_cases
    assert np.allclose(par[:, 0], case['charge'], rtol=0, atol=1e-12)
    assert np.array_equal(par[:, 1], case['radius']) and np.array_equal(par[:, 2], case['scale'])
    assert (gb.getSoluteDielectric(), gb.getSolventDielectric()) == (1.0, 78.3)
    # the System's method, cutoff and dielectrics
    system = heaq_forcefield().createSystem(pdb.topology, nonbondedMethod=app.CutoffNonPeriodic, nonbondedCutoff=0.9 * unit.nanometer,
                                            soluteDielectric=2.0, solventDielectric=80.0)
    (gb,) = [f for f in system.getForces() if isinstance(f, openmm.GBSAOBCForce)]
    assert gb.getNonbondedMethod() == gb.CutoffNonPeriodic and gb.getCutoffDistance()._value == 0.9
    assert (gb.getSoluteDielectric(), gb.getSolventDielectric()) == (2.0, 80.0)
    # a file without the section makes no such force
    plain = app.ForceField(os.path.join(GOLDEN, 'data', 'hydroxyethylaminoanthraquinone-in-water.xml')).createSystem(pdb.topology)
    assert not any(isinstance(f, openmm.GBSAOBCForce) for f in plain.getForces())


def test_forcefield_section_with_charges_of_its_own(tmp_path):
    text = """<ForceField>
 <AtomTypes><Type name="A" class="a" element="C" mass="12.0"/><Type name="B" class="b" element="H" mass="1.0"/></AtomTypes>
 <Residues><Residue name="XY"><Atom name="X" type="A" charge="9"/><Atom name="Y" type="B" charge="9"/><Bond from="0" to="1"/></Residue></Residues>
 <GBSAOBCForce><Atom type="A" charge="0.3" radius="0.17" scale="0.72"/><Atom class="b" charge="-0.3" radius="0.12" scale="0.85"/></GBSAOBCForce>
</ForceField>"""
    path = tmp_path / 'xy.xml'
    path.write_text(text)
    top = app.Topology()
    chain = top.addChain()
    res = top.addResidue('XY', chain)
    x = top.addAtom('X', None, res)
    y = top.addAtom('Y', None, res)
    top.addBond(x, y)
    system = app.ForceField(str(path)).createSystem(top)
    (gb,) = [f for f in system.getForces() if isinstance(f, openmm.GBSAOBCForce)]
    assert [[p[0]._value, p[1]._value, p[2]] for p in (gb.getParticleParameters(k) for k in range(2))] == [[0.3, 0.17, 0.72], [-0.3, 0.12, 0.85]]
    (path2 := tmp_path / 'nocharge.xml').write_text(text.replace(' charge="0.3"', ''))
    with pytest.raises(ValueError, match='no charge for atom type A'):
        app.ForceField(str(path2)).createSystem(top)


# ------------------------------------------------------------------------------------ what the engine hands over
def test_translation_groups_and_update(cases, heaq, recorder):
    case = G.s33(heaq)
    system = system_from_arrays(case, nonbondedMethod='NoCutoff')
    gb = add_gb(system, case)
    gb.setForceGroup(2)
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    rec = recorder[-1]
    assert context._engine.free_space and rec.box is None
    (made,) = rec.gbs
    assert np.array_equal(made['q'], case['charge']) and np.array_equal(made['radius'], cases['S33']['radius'])
    assert np.array_equal(made['scale'], cases['S33']['scale'])
    assert (made['eps_in'], made['eps_out'], made['sa_energy'], made['rc']) == (1.0, 78.3, 2.25936, 0.0)
    (entry,) = [e for e in context._engine.entries if e.force is gb]
    assert entry.gb == made['id'] and entry.term_ids == [made['id']] and not entry.pair_ids and entry.bonded_id is None
    # getState(groups=...) reaches it as a member of its group
    context.setPositions(case['positions'])
    context.getState(getForces=True, groups={2})
    assert [c for c in rec.calls if c[0] == 'force_eval'] == [('force_eval', made['id'], True)]
    context.getState(getForces=True, groups={0})
    assert [c for c in rec.calls if c[0] == 'force_eval'].count(('force_eval', made['id'], True)) == 1
    # updateParametersInContext: everything again
    gb.setParticleParameters(0, 0.5, 0.2, 0.9)
    gb.setSolventDielectric(80.0)
    gb.setSoluteDielectric(2.0)
    gb.setSurfaceAreaEnergy(3.0)
    gb.updateParametersInContext(context)
    (call,) = [c for c in rec.calls if c[0] == 'gb_set_params']
    assert call[1] == made['id'] and (call[2][0], call[3][0], call[4][0]) == (0.5, 0.2, 0.9) and np.array_equal(call[2][1:], case['charge'][1:])
    assert call[5:] == (2.0, 80.0, 3.0, 0.0)


def test_cutoff_non_periodic_and_a_system_of_gb_alone(cases, heaq, recorder):
    case = G.s33(heaq)
    system = system_from_arrays(case, nonbondedMethod='CutoffNonPeriodic', cutoff=1.0)
    add_gb(system, case, method=openmm.GBSAOBCForce.CutoffNonPeriodic, cutoff=0.8)
    openmm.Context(system, openmm.VerletIntegrator(0.001))
    assert recorder[-1].gbs[0]['rc'] == 0.8
    alone = openmm.System()
    for m in case['mass']:
        alone.addParticle(float(m))
    add_gb(alone, case)
    context = openmm.Context(alone, openmm.VerletIntegrator(0.001))
    assert context._engine.free_space and len(recorder[-1].gbs) == 1 and not recorder[-1].pairs


def test_a_respa_group_with_gb_takes_the_plain_path(cases, heaq, recorder):
    """RespaPropagator([2, 1]) with the bonded and pair forces in group 0 and the GB force in group 1: its group is evaluated by an
    EVAL op of its own, a member the scheduler's fusion rules decline (csrc/run_ops.hip takes bond-list sets and pair forces only)."""
    case = G.s33(heaq)
    system = system_from_arrays(case, nonbondedMethod='NoCutoff')
    add_gb(system, case).setForceGroup(1)
    integrator = atomsmm.RespaPropagator([2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(system, integrator)
    context.setPositions(case['positions'])
    context.setVelocitiesToTemperature(300 * unit.kelvin, 1)
    integrator.step(1)
    rec = recorder[-1]
    gid = rec.gbs[0]['id']
    assert rec.groups[1][1] == [gid] and gid not in rec.groups[0][1]
    evals = [op for ops, _ in rec.runs for op in ops if op[0] == B.OP_EVAL]
    assert any(op[1] == 1 for op in evals) and any(op[1] == 0 for op in evals)


# ------------------------------------------------------------------------------------ refusals, by name
def test_refusals(cases, heaq, spcfw, recorder):
    case = G.s33(heaq)
    verlet = lambda: openmm.VerletIntegrator(0.001)      # noqa: E731
    # CutoffPeriodic
    system = system_from_arrays(case, nonbondedMethod='NoCutoff')
    add_gb(system, case, method=openmm.GBSAOBCForce.CutoffPeriodic)
    with pytest.raises(atomsmm.InputError, match='GBSAOBCForce: CutoffPeriodic is not supported'):
        openmm.Context(system, verlet())
    # a box-periodic pair force in the System
    water = G.d1527(spcfw)
    system = system_from_arrays(dict(water, box=np.full(3, 4.0)), nonbondedMethod='CutoffPeriodic')
    add_gb(system, water, method=openmm.GBSAOBCForce.CutoffNonPeriodic)
    with pytest.raises(atomsmm.InputError, match='a GBSAOBCForce in a System with a box-periodic NonbondedForce'):
        openmm.Context(system, verlet())
    # the particle count
    system = system_from_arrays(case, nonbondedMethod='NoCutoff')
    add_gb(system, dict(case, mass=case['mass'][:32], charge=case['charge'][:32]))
    with pytest.raises(openmm.OpenMMException, match='GBSAOBCForce must have exactly as many particles as the System'):
        openmm.Context(system, verlet())
    # the virial
    system = system_from_arrays(dict(water, box=np.full(3, 4.0)), nonbondedMethod='CutoffPeriodic')
    add_gb(system, water)
    with pytest.raises(NotImplementedError, match='the virial of a GBSAOBCForce'):
        atomsmm.ComputingSystem(system)
    with pytest.raises(NotImplementedError, match='the virial of a GBSAOBCForce'):
        atomsmm.PressureComputer(system, app.Topology(1527), openmm.Platform.getPlatformByName('HIP'))
    # deriv(energy, .): when the Context is created, and from the engine
    system = system_from_arrays(case, nonbondedMethod='NoCutoff')
    add_gb(system, case)
    custom = openmm.CustomIntegrator(0.001)
    custom.addGlobalVariable('g', 0.0)
    custom.addComputeGlobal('g', 'deriv(energy, lambda_coul)')
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, ...\) through a GBSAOBCForce'):
        openmm.Context(system, custom)
    context = openmm.Context(system, verlet())
    with pytest.raises(NotImplementedError, match=r'deriv\(energy, lambda\) through a GBSAOBCForce'):
        context._engine.energy_derivative('lambda')
    # more than one rank

    def job(rank):
        with pytest.raises(atomsmm.InputError, match='a GBSAOBCForce runs on a single rank'):
            openmm.Context(copy.deepcopy(system), verlet())
        return True
    assert E.LocalWorld(2).run(job) == [True, True]


def test_the_size_limit_is_named(recorder):
    n = 32769
    system = openmm.System()
    for _ in range(n):
        system.addParticle(1.0)
    gb = openmm.GBSAOBCForce()
    gb._particles = [[0.0, 0.15, 0.8]] * n
    system.addForce(gb)
    with pytest.raises(atomsmm.InputError, match='GBSAOBCForce .* at most 32768 atoms'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))


def test_backend_exports_the_four_entry_points():
    for name in ('amm_gb_create', 'amm_gb_set_params', 'amm_gb_born_radii', 'amm_gb_release'):
        assert name in B.EXPORTS
    for name in ('gb_create', 'gb_set_params', 'gb_born_radii', 'gb_release'):
        assert callable(getattr(B.HipContext, name))
