"""GPU tests of CMAPTorsionForce (csrc/cmap.hip: one lane per term, bicubic patch of 16 coefficients per cell, parked forces gathered
per atom in record order) and of RBTorsionForce (lowered to the term-expression kernel).

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|.  The reference is
tests/cmap_cases.py: the tensor-product periodic cubic spline evaluated with scipy, dihedrals and their gradients in numpy fp64 --
independent of atomsmm_amd.tables and of the 16-coefficient form.  Map values lie in [1, 3] kJ/mol wherever a total is compared.
Every test prints its worst deviation; DESIGN.md 3.CM has the figures measured on an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import cmap_cases as C  # noqa: E402
from atomsmm_amd import engine as E  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402

E_REL, F_REL = 1e-10, 1e-9
BOX = np.full(3, 4.0)
MAPS = [C.random_map(5, 21), C.random_map(24, 22)]


def assert_close(e, f, e_ref, f_ref, what):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= E_REL * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


def cmap_force(maps, terms, periodic=False, group=0):
    force = openmm.CMAPTorsionForce()
    for size, energy in maps:
        force.addMap(size, energy)
    for row in terms:
        force.addTorsion(*[int(v) for v in row])
    force.setUsesPeriodicBoundaryConditions(periodic)
    force.setForceGroup(group)
    return force


def bare_system(n, box=None, mass=12.0):
    system = openmm.System()
    for _ in range(n):
        system.addParticle(mass)
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


# ------------------------------------------------------------------------------------ 1. lane layouts
@pytest.mark.parametrize('n_terms', [1, 63, 64, 65, 257])
def test_lane_layouts(n_terms):
    """On the parent commit: AttributeError, openmm has no CMAPTorsionForce.  Disjoint sets of eight atoms, maps of sizes 5 and 24
    assigned alternately: a partial wave, a full one, one lane into the next, more than one block."""
    pos, terms = C.disjoint_terms(n_terms, seed=30 + n_terms)
    ref = C.evaluate(pos, MAPS, terms)
    e, f, _ = one_force(len(pos), BOX, cmap_force(MAPS, terms), pos)
    assert_close(e, f, ref['energy'], ref['forces'], '%d disjoint terms' % n_terms)


# ------------------------------------------------------------------------------------ 2. shared atoms
def test_backbone_pattern_and_a_torsion_named_twice():
    """A chain of 70 atoms with the terms (k .. k+3, k+1 .. k+4): an inner atom collects up to eight records, three atoms of every
    term are named twice.  One more term names the same torsion for phi and for psi."""
    pos, terms = C.backbone(70, seed=41)
    terms = np.concatenate([terms, [[1, 10, 11, 12, 13, 10, 11, 12, 13]]])
    assert len(terms) == 67
    ref = C.evaluate(pos, MAPS, terms)
    e, f, context = one_force(70, None, cmap_force(MAPS, terms), pos)
    assert_close(e, f, ref['energy'], ref['forces'], 'backbone of 70 atoms, 66 + 1 terms')
    assert context._engine.free_space


# ------------------------------------------------------------------------------------ 3. nodes and wrap
def asymmetric_map(size=5):
    return 1.0 + np.arange(size * size) / float(size * size)


def quad(angle):
    """Four atoms with the dihedral `angle`."""
    return C.place_dihedral(angle, 0.0)[:4]


def planar_quad(cis, out_of_plane=0.0):
    """Four atoms in the plane z = 0 exactly, trans (dihedral pi) or cis (dihedral 0); the last atom lifted by `out_of_plane`."""
    y = 0.12 if cis else -0.12
    return np.array([[0.03, 0.12, 0.0], [0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.18, y, out_of_plane]])


def test_nodes_planar_geometries_and_cell_boundaries():
    """One term over two separate four-atom sets, one Context in free space, positions set again and again."""
    size = 5
    energy = asymmetric_map(size)
    delta = 2 * np.pi / size
    terms = [[0, 0, 1, 2, 3, 4, 5, 6, 7]]
    maps = [(size, energy)]
    system = bare_system(8)
    system.addForce(cmap_force(maps, terms))
    context = openmm.Context(system, openmm.VerletIntegrator(0.001))
    shift = np.array([0.0, 0.5, 0.0])        # (within the plane: z = 0 stays exact)

    def at(first, second):
        pos = np.concatenate([first, second + shift])
        context.setPositions(pos * unit.nanometers)
        e, f = energy_forces(context)
        return e, f, pos

    # all 25 nodes
    worst = 0.0
    for i in range(size):
        for j in range(size):
            e, _, _ = at(quad(i * delta), quad(j * delta))
            worst = max(worst, abs(e - energy[i + size * j]) / energy[i + size * j])
            assert abs(e - energy[i + size * j]) <= E_REL * energy[i + size * j]
    print('25 nodes of an asymmetric 5 x 5 map: worst rel deviation from energy[i + 5 j] %.2e' % worst)
    # phi = pi exactly: planar trans
    e, f, pos = at(planar_quad(cis=False), quad(1.0))
    assert abs(abs(C.dihedral(pos, [0, 1, 2, 3])[0]) - np.pi) == 0.0
    ref = C.evaluate(pos, maps, terms)
    assert_close(e, f, ref['energy'], ref['forces'], 'planar trans (phi = pi)')
    # planar cis with the last atom 1e-18 nm out of plane on the side of negative angles: -1e-18 + 2 pi rounds to 2 pi, cell index == size
    for lift in (1e-18, -1e-18):
        if C.dihedral(planar_quad(True, lift), [0, 1, 2, 3])[0] < 0.0:
            break
    tiny = C.dihedral(planar_quad(True, lift), [0, 1, 2, 3])[0]
    assert tiny < 0.0 and tiny + 2 * np.pi == 2 * np.pi
    e, f, pos = at(planar_quad(True, lift), planar_quad(True, lift))
    print('planar cis, last atom %.0e nm out of plane (angle %.3e): E = %.17g, node 0 holds %.17g' % (lift, tiny, e, energy[0]))
    assert np.isfinite(e) and np.isfinite(f).all() and abs(e - energy[0]) <= E_REL * energy[0]
    e, f, pos = at(planar_quad(True, lift), quad(2 * delta))
    assert np.isfinite(f).all() and abs(e - energy[0 + size * 2]) <= E_REL * energy[size * 2]
    # every cell boundary from both sides: the same energy, and that of the reference
    eps, worst = 1e-12, 0.0
    for k in range(size):
        for first in (True, False):
            got = []
            for side in (-eps, eps):
                angle = k * delta + side
                e, f, pos = at(quad(angle), quad(1.0)) if first else at(quad(1.0), quad(angle))
                ref = C.evaluate(pos, maps, terms)
                assert abs(e - ref['energy']) <= E_REL * abs(ref['energy'])
                assert np.abs(f - ref['forces']).max() <= F_REL * np.abs(ref['forces']).max()
                got.append(e)
            worst = max(worst, abs(got[0] - got[1]) / abs(got[0]))
            # the map's slope is of order (max - min) / delta = 1 kJ/mol/rad: 2e-12 rad apart the energies differ by 1e-12 at the most
            assert abs(got[0] - got[1]) <= E_REL * abs(got[0])
    print('cell boundaries from both sides (1e-12 rad): worst rel difference %.2e' % worst)
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 4. the convention, against the hand-written kind
def test_sampled_map_against_two_periodic_torsion_forces():
    size, k1, p1, k2, p2 = 72, 2.0, 0.7, 1.5, -1.1
    grid = np.arange(size) * (2 * np.pi / size)
    phi_g, psi_g = np.meshgrid(grid, grid, indexing='ij')
    analytic = lambda phi, psi: k1 * (1 + np.cos(phi - p1)) + k2 * (1 + np.cos(2 * psi - p2))      # noqa: E731
    energy = analytic(phi_g, psi_g).T.reshape(-1)                  # energy[i + size * j]: phi index fastest
    pos, terms = C.backbone(12, seed=51, n_maps=1)
    e, f, _ = one_force(12, BOX, cmap_force([(size, energy)], terms), pos)
    system = bare_system(12, BOX)
    first, second = openmm.PeriodicTorsionForce(), openmm.PeriodicTorsionForce()
    for row in terms:
        first.addTorsion(*[int(v) for v in row[1:5]], 1, p1, k1)
        second.addTorsion(*[int(v) for v in row[5:9]], 2, p2, k2)
    system.addForce(first)
    system.addForce(second)
    e_ref, f_ref = energy_forces(context_with(system, pos))
    # what the spline itself is off from the analytic form at these angles, from the reference: per term in the energy, and per atom
    # through |dE/dangle| times the angle's gradient
    spline = C.MapSpline(size, energy)
    e_allow, f_allow = 0.0, np.zeros_like(pos)
    for row in terms:
        phi, gphi = C.dihedral(pos, row[1:5])
        psi, gpsi = C.dihedral(pos, row[5:9])
        s, s_phi, s_psi = spline(phi, psi)
        e_allow += abs(s - analytic(phi, psi))
        d_phi = abs(s_phi + k1 * np.sin(phi - p1))
        d_psi = abs(s_psi + 2 * k2 * np.sin(2 * psi - p2))
        for k in range(4):
            f_allow[row[1 + k]] += d_phi * np.abs(gphi[k])
            f_allow[row[5 + k]] += d_psi * np.abs(gpsi[k])
    scale = np.abs(f_ref).max()
    print('72 x 72 sampled map against two PeriodicTorsionForces: |dE| = %.3e (the spline is off by %.3e, E = %.6g), max|dF| = %.3e '
          '(the spline by up to %.3e, max|F| = %.6g)' % (abs(e - e_ref), e_allow, e_ref, np.abs(f - f_ref).max(), f_allow.max(), scale))
    assert abs(e - e_ref) <= e_allow + E_REL * abs(e_ref)
    assert np.all(np.abs(f - f_ref) <= f_allow + F_REL * scale)
    assert e_allow < 1e-4 * abs(e_ref)          # (the map is fine enough that a swapped axis or a shifted origin could not hide: k1 != k2, p1 != p2)


# ------------------------------------------------------------------------------------ 5. minimum image
def test_terms_across_a_box_face():
    box = np.full(3, 3.0)
    pos, terms = C.backbone(20, seed=61, start=(2.9, 1.5, 0.05))
    wrapped = pos - box * np.floor(pos / box)
    assert (np.abs(wrapped - pos).max(axis=0) > 0).any() and np.abs(wrapped[1:] - wrapped[:-1]).max() > 1.5     # bonds do straddle faces
    ref = C.evaluate(pos, MAPS, terms)
    e, f, _ = one_force(20, box, cmap_force(MAPS, terms, periodic=True), wrapped)
    assert_close(e, f, ref['energy'], ref['forces'], 'terms across box faces, periodic')
    images = C.evaluate(wrapped, MAPS, terms, box=box)
    assert abs(images['energy'] - ref['energy']) <= 1e-12 * abs(ref['energy'])


# ------------------------------------------------------------------------------------ 6. updateParametersInContext
def test_update_parameters_matches_a_fresh_context():
    pos, terms = C.backbone(40, seed=71)
    force = cmap_force(MAPS, terms)
    e0, f0, context = one_force(40, BOX, force, pos)
    fresh_maps = [C.random_map(5, 72), MAPS[1]]
    fresh_terms = terms.copy()
    fresh_terms[::3, 0] = 1 - fresh_terms[::3, 0]
    force.setMapParameters(0, *fresh_maps[0])
    for k, row in enumerate(fresh_terms):
        force.setTorsionParameters(k, *[int(v) for v in row])
    force.updateParametersInContext(context)
    e1, f1 = energy_forces(context)
    e2, f2, _ = one_force(40, BOX, cmap_force(fresh_maps, fresh_terms), pos)
    ref = C.evaluate(pos, fresh_maps, fresh_terms)
    assert_close(e1, f1, ref['energy'], ref['forces'], 'after updateParametersInContext')
    assert e1 == e2 and np.array_equal(f1, f2) and e1 != e0
    # what may not change is refused and leaves the Context as it was
    force.addTorsion(0, 0, 1, 2, 3, 1, 2, 3, 4)
    with pytest.raises(openmm.OpenMMException, match='the number of torsions has changed'):
        force.updateParametersInContext(context)
    e3, f3 = energy_forces(context)
    assert e3 == e1 and np.array_equal(f3, f1)


# ------------------------------------------------------------------------------------ 7. determinism
def test_same_bits_with_and_without_energy_and_accumulate():
    pos, terms = C.backbone(70, seed=81)
    _, _, context = one_force(70, BOX, cmap_force(MAPS, terms), pos)
    ctx = context._engine.ctx
    (fid,) = [e.cmap for e in context._engine.entries if e.cmap is not None]
    e1, f1 = evaluate(ctx, fid, pos)
    e2, f2 = evaluate(ctx, fid, pos)
    _, f3 = evaluate(ctx, fid, pos, energy=False)
    assert e1 == e2 and np.array_equal(f1, f2) and np.array_equal(f1, f3) and np.abs(f1).max() > 1.0
    start = np.random.default_rng(82).normal(size=pos.shape) * 50.0
    e4, f4 = evaluate(ctx, fid, pos, accumulate=True, start=start)
    assert e4 == e1 and np.array_equal(f4, start + f1)
    # without accumulate every row is written: atoms in no term come out zero from a pre-filled buffer
    lone = np.concatenate([pos, [[3.5, 3.5, 3.5]]])
    _, _, context = one_force(71, BOX, cmap_force(MAPS, terms), lone)
    (fid,) = [e.cmap for e in context._engine.entries if e.cmap is not None]
    _, f5 = evaluate(context._engine.ctx, fid, lone, start=np.full((71, 3), 7.0))
    assert np.array_equal(f5[:70], f1) and not f5[70].any()
    ctx.check()


def test_the_backend_refuses_what_the_header_says():
    from atomsmm_amd import backend as B
    from atomsmm_amd import tables as T
    coeffs = T.cmap_coefficients(*MAPS[0]).reshape(-1)
    ctx = B.HipContext(8, BOX)
    try:
        idx = [[0, 1, 2, 3, 4, 5, 6, 7]]
        with pytest.raises(B.HipError, match='atom index 8 of term 0 is out of range'):
            ctx.cmap_create([5], coeffs, [0], [[0, 1, 2, 3, 4, 5, 6, 8]])
        with pytest.raises(B.HipError, match='names map 1'):
            ctx.cmap_create([5], coeffs, [1], idx)
        with pytest.raises(B.HipError, match='map 0 has size 1'):
            ctx.cmap_create([1], coeffs[:16], [0], idx)
        fid = ctx.cmap_create([5], coeffs, [0], idx, periodic=True)
        with pytest.raises(B.HipError, match='names map 3'):
            ctx.cmap_set_params(fid, coeffs, [3], 1)
        with pytest.raises(B.HipError, match='1 maps and 1 terms, 2 and 1 given'):
            ctx.cmap_set_params(fid, coeffs, [0], 2)
        with pytest.raises(B.HipError, match='384 coefficients given, the force was created with 400'):
            ctx.cmap_set_params(fid, coeffs[:-16], [0], 1)
        # the other families name the type
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.pair_stats(fid)
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.bonded_finalize(fid)
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.term_expr_set_params(fid, np.zeros((1, 1)), 1)
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.compound_set_params(fid, np.zeros((1, 1)), 1)
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.pme_set_charges(fid, np.zeros(8))
        with pytest.raises(B.HipError, match='AMM_FORCE_CMAP'):
            ctx.cv_create([fid], 0, [0], [], [])
        ctx.cmap_release(fid)
        with pytest.raises(B.HipError, match='not the id of a CMAP force'):
            ctx.cmap_release(fid)
    finally:
        ctx.close()
    free = B.HipContext(8, None)
    try:
        with pytest.raises(B.HipError, match='the context has no periodic box'):
            free.cmap_create([5], coeffs, [0], idx, periodic=True)
    finally:
        free.close()


# ------------------------------------------------------------------------------------ 8. integration
def test_get_state_isolates_the_cmap_group():
    pos, terms = C.backbone(30, seed=91)
    system = bare_system(30, BOX)
    bonds = openmm.HarmonicBondForce()
    for k in range(29):
        bonds.addBond(k, k + 1, 0.14, 2.0e4)
    system.addForce(bonds)
    system.addForce(cmap_force(MAPS, terms, group=2))
    context = context_with(system, pos)
    ref = C.evaluate(pos, MAPS, terms)
    e, f = energy_forces(context, groups={2})
    assert_close(e, f, ref['energy'], ref['forces'], 'getState(groups={2})')
    e_all, f_all = energy_forces(context)
    e_bonds, f_bonds = energy_forces(context, groups={0})
    assert abs(e_all - (e + e_bonds)) <= 1e-12 * abs(e_all) and np.abs(f_all - (f + f_bonds)).max() <= 1e-12 * np.abs(f_all).max()
    assert e_bonds > 0.0


def thermal_velocities(data, seed=2026):
    kT = unit.MOLAR_GAS_CONSTANT_R._value * 300.0
    return np.random.default_rng(seed).normal(size=data['positions'].shape) * np.sqrt(kT / data['mass'])[:, None]


def test_four_respa_steps_fusion_on_and_off(spcfw):
    """64 CMAP terms over runs of five consecutive atoms of flexible water (periodic), in the innermost group of RESPA [4, 2, 1]: the
    fusion rules decline the group, it is evaluated member by member, and the steps end at the same bits with fusion on and off."""
    terms = np.array([[k % 2, 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3, 3 * k + 1, 3 * k + 2, 3 * k + 3, 3 * k + 4] for k in range(64)])
    results = []
    for fuse in (True, False):
        system = atomsmm.RESPASystem(system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic'), 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        system.addForce(cmap_force(MAPS, terms, periodic=True, group=0))
        integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
        context = context_with(system, spcfw['positions'], integrator)
        context.setVelocities(thermal_velocities(spcfw))
        context._engine.ctx.set_fuse_inner(fuse)
        assert [(type(e.force).__name__, e.group) for e in context._engine.entries if e.cmap is not None] == [('CMAPTorsionForce', 0)]
        integrator.step(4)
        results.append((positions_of(context), context._engine.ctx.run_stats()))
        context._engine.ctx.check()
    (x_on, stats_on), (x_off, stats_off) = results
    print('4 RESPA [4, 2, 1] steps with CMAP innermost: run statistics with fusion %s, without %s' % (stats_on, stats_off))
    assert np.array_equal(x_on, x_off) and stats_on['epilogues'] == 0 and stats_off['epilogues'] == 0
    assert np.abs(x_on - spcfw['positions']).max() > 1e-4


def single_well(size, phi0, psi0, depth=40.0):
    grid = np.arange(size) * (2 * np.pi / size)
    phi, psi = np.meshgrid(grid, grid, indexing='ij')
    return size, (1.0 + depth * (1.0 - 0.5 * (np.cos(phi - phi0) + np.cos(psi - psi0)))).T.reshape(-1)


def five_atom_chain(well):
    system = bare_system(5)
    bonds, angles = openmm.HarmonicBondForce(), openmm.HarmonicAngleForce()
    for k in range(4):
        bonds.addBond(k, k + 1, 0.15, 2.0e5)
    for k in range(3):
        angles.addAngle(k, k + 1, k + 2, np.deg2rad(111.0), 400.0)
    system.addForce(bonds)
    system.addForce(angles)
    system.addForce(cmap_force([well], [[0, 0, 1, 2, 3, 1, 2, 3, 4]]))
    return system


def angles_of(x):
    return np.mod([C.dihedral(x, [0, 1, 2, 3])[0], C.dihedral(x, [1, 2, 3, 4])[0]], 2 * np.pi)


def test_verlet_steps_and_minimisation_end_in_the_well():
    """One term with a single-well 24 x 24 map on a five-atom chain in free space (bonds and angles at rest): 20 stock Verlet steps
    from rest move downhill, minimizeEnergy ends in the well's cell."""
    size, delta = 24, 2 * np.pi / 24
    phi0, psi0 = 18.5 * delta, 7.5 * delta            # the middle of cell (18, 7)
    well = single_well(size, phi0, psi0)
    start = C.place_dihedral(phi0 + 1.2, psi0 - 0.9) + 1.0
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(five_atom_chain(well), start, integrator)
    assert context._engine.free_space
    pe0 = context.getState(getEnergy=True).getPotentialEnergy()._value
    integrator.step(20)
    state = context.getState(getEnergy=True)
    pe1, ke1 = state.getPotentialEnergy()._value, state.getKineticEnergy()._value
    print('20 Verlet steps from rest: PE %.6f -> %.6f, KE %.6f, PE + KE off by %.2e' % (pe0, pe1, ke1, pe1 + ke1 - pe0))
    assert pe1 < pe0 and ke1 > 0.0 and np.isfinite(pe1)
    context._engine.ctx.check()
    sim = app.Simulation(app.Topology(5), five_atom_chain(well), openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(start * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy()
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    before, after = angles_of(start), angles_of(positions_of(sim.context))
    print('minimisation: E %.6f -> %.6f; (phi, psi) / delta %s -> %s, the well is in cell (18, 7)' % (e0, e1, before / delta, after / delta))
    assert e1 < e0 and (np.floor(before / delta) != [18, 7]).all() and (np.floor(after / delta) == [18, 7]).all()
    sim.context._engine.ctx.check()


def test_a_virtual_site_among_the_eight_atoms():
    """Atom 4 of the term is a TwoParticleAverageSite of atoms 5 and 6: its force is spread to them, the total force stays zero."""
    rng = np.random.default_rng(95)
    pos = np.concatenate([C.chain(rng, 5, start=(1.0, 1.0, 1.0)), np.zeros((2, 3))])
    pos[5] = pos[4] + [0.05, -0.02, 0.03]
    pos[6] = pos[4] - np.array([0.05, -0.02, 0.03]) * 0.3 / 0.7
    terms = [[1, 0, 1, 2, 3, 1, 2, 3, 4]]
    system = bare_system(7)
    system.setParticleMass(4, 0.0)
    system.setVirtualSite(4, openmm.TwoParticleAverageSite(5, 6, 0.3, 0.7))
    system.addForce(cmap_force(MAPS, terms))
    context = context_with(system, pos)
    context.computeVirtualSites()
    x = positions_of(context)
    assert np.abs(x[4] - pos[4]).max() <= 1e-15 * 2
    e, f = energy_forces(context)
    ref = C.evaluate(x, MAPS, terms)
    want = ref['forces'].copy()
    want[5] += 0.3 * want[4]
    want[6] += 0.7 * want[4]
    want[4] = 0.0
    assert_close(e, f, ref['energy'], want, 'a virtual site as the last atom of psi')
    scale = np.abs(want).max()
    print('total force %.3e of max|F| = %.6g' % (np.abs(f.sum(axis=0)).max() / scale, scale))
    assert np.abs(ref['forces'][4]).max() > 1e-3 * scale and not f[4].any()
    assert np.abs(f.sum(axis=0)).max() <= F_REL * scale


# ------------------------------------------------------------------------------------ 9. RBTorsionForce
def rb_case(n=70, seed=97):
    pos, _ = C.backbone(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    rows = [(k, k + 1, k + 2, k + 3) for k in range(n - 3)]
    coef = rng.uniform(-5.0, 5.0, (len(rows), 6))
    coef[:, 0] = rng.uniform(20.0, 30.0, len(rows))          # (the total stays far from zero)
    return pos, rows, coef


def test_rb_against_the_closed_form():
    """On the parent commit: AttributeError, openmm has no RBTorsionForce."""
    pos, rows, coef = rb_case()
    force = openmm.RBTorsionForce()
    for row, c in zip(rows, coef):
        force.addTorsion(*row, *[float(v) for v in c])
    e, f, context = one_force(len(pos), BOX, force, pos)
    e_ref, f_ref = 0.0, np.zeros_like(pos)
    for row, c in zip(rows, coef):
        phi, grad = C.dihedral(pos, row)
        cp = np.cos(phi - np.pi)
        e_ref += sum(c[n] * cp ** n for n in range(6))
        de_dphi = sum(n * c[n] * cp ** (n - 1) for n in range(1, 6)) * -np.sin(phi - np.pi)
        for k in range(4):
            f_ref[row[k]] -= de_dphi * grad[k]
    assert_close(e, f, e_ref, f_ref, '67 Ryckaert-Bellemans torsions against sum c_n cos(phi - pi)^n')
    # bit for bit the CustomTorsionForce with the same text
    twin = openmm.CustomTorsionForce(E.Engine.RB_TEXT)
    for k in range(6):
        twin.addPerTorsionParameter('c%d' % k)
    for row, c in zip(rows, coef):
        twin.addTorsion(*row, [float(v) for v in c])
    e2, f2, _ = one_force(len(pos), BOX, twin, pos)
    assert e == e2 and np.array_equal(f, f2)
    # updateParametersInContext follows new coefficients
    force.setTorsionParameters(0, *rows[0], *[float(v) for v in coef[0] + 1.0])
    force.updateParametersInContext(context)
    e3, _ = energy_forces(context)
    phi = C.dihedral(pos, rows[0])[0]
    assert e3 - e == pytest.approx(sum(np.cos(phi - np.pi) ** n for n in range(6)), rel=1e-9)


def test_forcefield_system_minimises_and_runs_npt_and_respa(tmp_path):
    """A System read from force-field XML with <CMAPTorsionForce> and <RBTorsionForce>: minimizeEnergy, NPT with
    LangevinMiddleIntegrator, and RESPA, as a script written for OpenMM would run them."""
    field = """<ForceField>
 <AtomTypes><Type name="tC" class="C" element="C" mass="12.0"/><Type name="tN" class="N" element="N" mass="14.0"/></AtomTypes>
 <Residues><Residue name="PEN"><Atom name="A1" type="tC" charge="0.1"/><Atom name="A2" type="tN" charge="-0.1"/><Atom name="A3" type="tC" charge="0.1"/>
  <Atom name="A4" type="tC" charge="-0.2"/><Atom name="A5" type="tN" charge="0.1"/>
  <Bond from="0" to="1"/><Bond from="1" to="2"/><Bond from="2" to="3"/><Bond from="3" to="4"/></Residue></Residues>
 <HarmonicBondForce><Bond class1="C" class2="N" length="0.14" k="2.0e5"/><Bond class1="C" class2="C" length="0.15" k="2.0e5"/></HarmonicBondForce>
 <HarmonicAngleForce><Angle class1="" class2="" class3="" angle="1.94" k="400.0"/></HarmonicAngleForce>
 <RBTorsionForce><Proper class1="" class2="N" class3="C" class4="" c0="3.0" c1="-1.0" c2="0.5" c3="0.2" c4="-0.1" c5="0.05"/></RBTorsionForce>
 <CMAPTorsionForce><Map>%s</Map><Torsion map="0" class1="C" class2="N" class3="C" class4="C" class5="N"/></CMAPTorsionForce>
 <NonbondedForce coulomb14scale="0.5" lj14scale="0.5"><UseAttributeFromResidue name="charge"/>
  <Atom class="C" sigma="0.34" epsilon="0.36"/><Atom class="N" sigma="0.325" epsilon="0.71"/></NonbondedForce>
</ForceField>""" % ' '.join('%.6f' % v for v in single_well(12, 1.0, 2.0, depth=5.0)[1])
    (path := tmp_path / 'pen.xml').write_text(field)
    top = app.Topology()
    chain = top.addChain()
    rng = np.random.default_rng(99)
    pos = []
    side = 4
    for cell in range(side ** 3):
        res = top.addResidue('PEN', chain)
        atoms = [top.addAtom('A%d' % k, None, res) for k in range(1, 6)]
        for a, b in zip(atoms[:-1], atoms[1:]):
            top.addBond(a, b)
        origin = 0.9 * np.array([cell % side, (cell // side) % side, cell // side ** 2]) + 0.3
        pos.append(C.place_dihedral(rng.uniform(-3, 3), rng.uniform(-3, 3)) + origin)
    pos = np.concatenate(pos)
    top.setUnitCellDimensions((0.9 * side,) * 3)
    forcefield = app.ForceField(str(path))

    def make_system():
        return forcefield.createSystem(top, nonbondedMethod=app.CutoffPeriodic, nonbondedCutoff=1.0 * unit.nanometers, removeCMMotion=False)

    system = make_system()
    (cmap,) = [f for f in system.getForces() if isinstance(f, openmm.CMAPTorsionForce)]
    (rb,) = [f for f in system.getForces() if isinstance(f, openmm.RBTorsionForce)]
    assert cmap.getNumTorsions() == side ** 3 and rb.getNumTorsions() == side ** 3
    barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 5)
    barostat.setRandomNumberSeed(11)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(3)
    sim = app.Simulation(top, system, integrator, openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(pos * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy(maxIterations=50)
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.context.setVelocitiesToTemperature(300.0, 5)
    sim.step(20)
    e2 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    print('force-field System of %d atoms: E %.4f -> %.4f (minimised) -> %.4f after 20 NPT steps' % (len(pos), e0, e1, e2))
    assert e1 < e0 and np.isfinite(e2)
    sim.context._engine.ctx.check()
    respa = atomsmm.RESPASystem(make_system(), 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
    context = context_with(respa, positions_of(sim.context), integrator)
    context.setVelocitiesToTemperature(300.0, 5)
    integrator.step(4)
    e3 = context.getState(getEnergy=True).getPotentialEnergy()._value
    print('4 RESPA [4, 2, 1] steps: E = %.4f' % e3)
    assert np.isfinite(e3) and any(e.cmap is not None for e in context._engine.entries)
    context._engine.ctx.check()
