"""GPU tests of the compound-bond forces (csrc/compound.hip): CustomCompoundBondForce and CustomCentroidBondForce with any energy
text, one lane per (bond, variable), centres of groups ahead of the evaluation and a spread over their members behind it.

Tolerances are the project's own: energy rel 1e-10, forces 1e-9 of max|F|, 1e-12 nm for the short
trajectories, 1e-10 for collective-variable values.  References: tests/compound_cases.py (the text at 50 digits, forces by mpmath.diff
in the Cartesian coordinates of the atoms themselves), the CPU oracle and the hand-written GPU kinds for texts that restate one.

Worst deviations measured on an MI355X (every test prints its own): lane layouts V = 1, 2, 3, 5, 16 over 1, 15, 17,
65 bonds against the 50-digit reference -- energy rel 1.2e-14 (V = 1; 1.4e-15 beyond), forces 9.4e-15 of max|F| (V = 1; 3.2e-15
beyond); restated kinds over q-SPC-FW and emim-BCN4 against the oracle and the hand-written GPU kinds -- 1.1e-15 and 1.9e-13 (the
angles of emim against HarmonicAngleForce; 2.4e-15 elsewhere); Urey-Bradley against angle + 1-3 bond -- 0 and 1.9e-13; across a box
face -- 5.0e-15 and 1.0e-14; centres over groups of 1, 3, 64, 65 atoms -- 5.1e-16 and 2.4e-15; the centre of 130 atoms -- rel
2.4e-16, its forces 7.5e-16 and 5.6e-16; single-atom groups of weight 1 against the compound bond -- the same bits; CustomCVForce
over a centroid distance / a compound dihedral against the direct texts -- 0 and 1.4e-16; 20 Verlet steps against the harmonic kinds
-- 1.2e-14 nm; 4 RESPA [4, 2, 1] steps with fusion on and off -- the same bits, 0 epilogue launches; minimisation -- the distance
between two centres 0.871 -> 0.6016 nm (d0 0.6, thermal width 0.05)."""
import math

import mpmath
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
import compound_cases as C  # noqa: E402
import expr_reference as R  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

E_REL, F_REL, X_ABS, D_REL = 1e-10, 1e-9, 1e-12, 1e-10
BOX = np.full(3, 4.0)


def assert_close(e, f, e_ref, f_ref, what, e_rel=E_REL):
    scale = np.abs(f_ref).max()
    print('%s: E = %.15g (reference %.15g, rel %.2e)  max|dF| = %.3e = %.2e of max|F| = %.6g' %
          (what, e, e_ref, abs(e - e_ref) / max(abs(e_ref), 1e-300), np.abs(f - f_ref).max(), np.abs(f - f_ref).max() / max(scale, 1e-300), scale))
    assert abs(e - e_ref) <= e_rel * abs(e_ref)
    assert np.abs(f - f_ref).max() <= F_REL * scale


def compound_force(name, rows, params, periodic=False, group=0, gvalues=None, text=None):
    case = C.TEXTS[name]
    force = openmm.CustomCompoundBondForce(case['n'], text or case['text'])
    for p in case['names']:
        force.addPerBondParameter(p)
    for g, value in (case['globals'] if gvalues is None else gvalues).items():
        force.addGlobalParameter(g, value)
    for members, row in zip(rows, params):
        force.addBond([int(a) for a in members], [float(v) for v in row])
    force.setUsesPeriodicBoundaryConditions(periodic)
    force.setForceGroup(group)
    return force


def centroid_force(name, groups, rows, params, periodic=False, gvalues=None):
    """groups: (atoms, weights or None for the masses); rows: group indices of every bond."""
    case = C.TEXTS[name]
    force = openmm.CustomCentroidBondForce(case['n'], case['text'])
    for p in case['names']:
        force.addPerBondParameter(p)
    for g, value in (case['globals'] if gvalues is None else gvalues).items():
        force.addGlobalParameter(g, value)
    for atoms, weights in groups:
        force.addGroup([int(a) for a in atoms], [] if weights is None else [float(w) for w in weights])
    for members, row in zip(rows, params):
        force.addBond([int(g) for g in members], [float(v) for v in row])
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


def bare_system(masses, box=None):
    system = openmm.System()
    for m in masses:
        system.addParticle(float(m))
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


def one_force(masses, box, force, positions):
    system = bare_system(masses, box)
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


def harmonic_rows(data):
    return {'harmonic-bond': (data['bonds'], np.stack([data['bond_r0'], data['bond_k']], axis=1)),
            'harmonic-angle': (data['angles'], np.stack([data['angle_theta0'], data['angle_k']], axis=1)),
            'periodic-torsion': (data['torsions'], np.stack([data['torsion_n'].astype(float), data['torsion_phase'], data['torsion_k']], axis=1))}


def with_groups(members, groups, masses):
    """Reference members of a centroid bond: (atoms, weights) per slot, the masses where a group has no weights."""
    return [(list(groups[g][0]), list(masses[list(groups[g][0])] if groups[g][1] is None else groups[g][1])) for g in members]


# ------------------------------------------------------------------------------------ 1. fails without the feature
def test_both_classes_run_in_a_context(spcfw):
    """On the parent commit: AttributeError, openmm has no CustomCompoundBondForce / CustomCentroidBondForce."""
    angles = spcfw['angles']
    rng = np.random.default_rng(1)
    par = np.stack([spcfw['angle_theta0'], spcfw['angle_k'], np.full(len(angles), 0.16), rng.uniform(1000, 3000, len(angles))], axis=1)
    e, f, context = one_force(spcfw['mass'], spcfw['box'], compound_force('urey-bradley', angles, par, periodic=True), spcfw['positions'])
    (entry,) = context._engine.entries
    assert entry.term_expr and len(entry.term_ids) == 1 and entry.bonded_id is None and entry.compound['variables'] == [('angle', (0, 1, 2)), ('distance', (0, 2))]
    assert math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1.0
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max()
    # two water molecules pulled together by their centres of mass
    groups = [(np.arange(0, 3), None), (np.arange(30, 33), None)]
    e, f, context = one_force(spcfw['mass'], spcfw['box'], centroid_force('centre-distance', groups, [[0, 1]], [[500.0, 0.3]]), spcfw['positions'])
    assert context._engine.entries[0].compound['centroid'] and math.isfinite(e) and e != 0.0 and np.isfinite(f).all() and np.abs(f).max() > 1.0
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).max() and not f[3:30].any() and not f[33:].any()


# ------------------------------------------------------------------------------------ 2. lane layouts
LAYOUTS = ('harmonic-bond', 'torsion-14', 'stretch-bend', 'five', 'sixteen')          # V = 1, 2, 3, 5, 16 -> L = 1, 2, 4, 8, 16
COUNTS = (1, 15, 17, 65)


@pytest.fixture(scope='module')
def layout_references(emim):
    """Per text: the 65 bonds, their parameters and the per-bond reference (computed once, never written to); a count takes a prefix."""
    made = {}

    def get(name):
        if name not in made:
            rows, params, looked = C.fixture_rows(name, emim, max(COUNTS))
            assert len(rows) >= C.MIN_KEPT * looked
            made[name] = (rows, params) + C.bond_sum(C.TEXTS[name], rows, params, emim['positions'], emim['box'])
        return made[name]
    return get


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('name', LAYOUTS)
def test_lane_layouts(layout_references, emim, name, count):
    rows, params, energies, forces = layout_references(name)
    assert C.N_VARIABLES[name] == {'harmonic-bond': 1, 'torsion-14': 2, 'stretch-bend': 3, 'five': 5, 'sixteen': 16}[name]
    e, f, context = one_force(emim['mass'], emim['box'], compound_force(name, rows[:count], params[:count], periodic=True), emim['positions'])
    assert len(context._engine.entries[0].compound['variables']) == C.N_VARIABLES[name]
    e_ref, f_ref = C.total(energies, forces, len(emim['positions']), count)
    assert_close(e, f, e_ref, f_ref, 'emim / %s (%d particles, %d variables), %d bonds' % (name, C.TEXTS[name]['n'], C.N_VARIABLES[name], count))


# ------------------------------------------------------------------------------------ 3. restated kinds, whole fixtures
ORACLE = {'harmonic-bond': lambda i, p, x, L, per: O.harmonic_bonds(i, p[:, 0], p[:, 1], x, L, periodic=per),
          'harmonic-angle': lambda i, p, x, L, per: O.harmonic_angles(i, p[:, 0], p[:, 1], x, L, periodic=per),
          'periodic-torsion': lambda i, p, x, L, per: O.periodic_torsions(i, p[:, 0].astype(np.int32), p[:, 1], p[:, 2], x, L, periodic=per)}


def hand_written_force(name, idx, params, periodic):
    if name == 'harmonic-bond':
        force = openmm.HarmonicBondForce()
        for (i, j), (r0, k) in zip(idx, params):
            force.addBond(int(i), int(j), float(r0), float(k))
    elif name == 'harmonic-angle':
        force = openmm.HarmonicAngleForce()
        for (i, j, k_), (t0, k) in zip(idx, params):
            force.addAngle(int(i), int(j), int(k_), float(t0), float(k))
    else:
        force = openmm.PeriodicTorsionForce()
        for (a, b, c, d), (n, phase, k) in zip(idx, params):
            force.addTorsion(int(a), int(b), int(c), int(d), int(n), float(phase), float(k))
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('fixture,name', [('spcfw', 'harmonic-bond'), ('spcfw', 'harmonic-angle'), ('emim', 'harmonic-bond'),
                                          ('emim', 'harmonic-angle'), ('emim', 'periodic-torsion')])
def test_restated_kinds_against_the_oracle_and_the_hand_written_kernels(request, fixture, name, periodic):
    data = request.getfixturevalue(fixture)
    idx, params = harmonic_rows(data)[name]
    assert len(idx) == {('spcfw', 'harmonic-bond'): 1024, ('spcfw', 'harmonic-angle'): 512, ('emim', 'harmonic-bond'): 2700,
                        ('emim', 'harmonic-angle'): 4300, ('emim', 'periodic-torsion'): 4100}[(fixture, name)]
    e, f, context = one_force(data['mass'], data['box'], compound_force(name, idx, params, periodic), data['positions'])
    assert context._engine.entries[0].compound is not None
    e_hand, f_hand, _ = one_force(data['mass'], data['box'], hand_written_force(name, idx, params, periodic), data['positions'])
    e_ref, f_ref = ORACLE[name](idx, params, data['positions'], data['box'], periodic)
    assert_close(e, f, e_ref, f_ref, '%s / %s, periodic %s, against the oracle' % (fixture, name, periodic))
    assert_close(e, f, e_hand, f_hand, '%s / %s, periodic %s, against the hand-written kind' % (fixture, name, periodic))


@pytest.mark.parametrize('periodic', [True, False])
def test_urey_bradley_is_the_sum_of_its_two_parts(emim, periodic):
    angles = emim['angles']
    rng = np.random.default_rng(2)
    d = emim['positions'][angles[:, 0]] - emim['positions'][angles[:, 2]]
    d -= emim['box'] * np.rint(d / emim['box'])
    d0, kub = np.sqrt((d * d).sum(axis=1)) + rng.uniform(-0.01, 0.01, len(angles)), rng.uniform(1000.0, 5000.0, len(angles))
    par = np.stack([emim['angle_theta0'], emim['angle_k'], d0, kub], axis=1)
    e, f, _ = one_force(emim['mass'], emim['box'], compound_force('urey-bradley', angles, par, periodic), emim['positions'])
    e_a, f_a, _ = one_force(emim['mass'], emim['box'], hand_written_force('harmonic-angle', angles, par[:, :2], periodic), emim['positions'])
    e_b, f_b, _ = one_force(emim['mass'], emim['box'], hand_written_force('harmonic-bond', angles[:, [0, 2]], par[:, 2:], periodic), emim['positions'])
    assert_close(e, f, e_a + e_b, f_a + f_b, 'emim / Urey-Bradley over %d angles, periodic %s, against angle + 1-3 bond' % (len(angles), periodic))


# ------------------------------------------------------------------------------------ 4. across a box face
def test_bonds_across_a_box_face():
    """Particles on both sides of the face x = 0 of a 4 nm box: with the flag, the numbers of the unwrapped copy; without it, those of
    the raw coordinates.  A text in x1 is never wrapped."""
    whole = np.array([[0.05, 1.0, 1.0], [-0.06, 1.08, 1.0], [-0.10, 1.20, 1.07], [0.02, 1.28, 1.15]])
    wrapped = whole.copy()
    wrapped[whole[:, 0] < 0, 0] += 4.0
    cases = [('harmonic-bond', [0, 1], [0.1, 3e5]), ('urey-bradley', [0, 1, 2], [1.9, 400.0, 0.2, 2000.0]),
             ('periodic-torsion', [0, 1, 2, 3], [2.0, 0.3, 12.0]), ('torsion-14', [0, 1, 2, 3], [3.0, 0.5, 8.0, 0.3, 900.0])]
    masses = [12.0] * 4
    for name, members, par in cases:
        case = C.TEXTS[name]
        on, off = compound_force(name, [members], [par], periodic=True), compound_force(name, [members], [par], periodic=False)
        e_ref, f_ref = C.total(*C.bond_sum(case, [members], [par], whole), 4)
        assert_close(*one_force(masses, BOX, off, whole)[:2], e_ref, f_ref, name + ', unwrapped copy')
        e_on, f_on, _ = one_force(masses, BOX, on, wrapped)
        assert_close(e_on, f_on, e_ref, f_ref, name + ', across the face with the flag')
        e_raw, f_raw = C.total(*C.bond_sum(case, [members], [par], wrapped), 4)
        e_off, f_off, _ = one_force(masses, BOX, off, wrapped)
        assert_close(e_off, f_off, e_raw, f_raw, name + ', across the face without the flag (raw distances)')
        assert abs(e_off - e_on) > 1e-3 * abs(e_on)
    force = openmm.CustomCompoundBondForce(2, 'k*(x1-x2)^2 + distance(p1,p2)')
    force.addGlobalParameter('k', 3.0)
    force.addBond([0, 1])
    force.setUsesPeriodicBoundaryConditions(True)
    e, f, _ = one_force(masses, BOX, force, wrapped)
    r = np.linalg.norm(whole[0] - whole[1])
    dx = wrapped[0, 0] - wrapped[1, 0]
    print('x1 - x2 with the flag: E = %.15g, raw coordinates give %.15g' % (e, 3.0 * dx * dx + r))
    assert e == pytest.approx(3.0 * dx * dx + r, rel=E_REL) and abs(dx) > 3.8
    assert f[0, 0] == pytest.approx(-6.0 * dx - (whole[0, 0] - whole[1, 0]) / r, rel=F_REL)


# ------------------------------------------------------------------------------------ 5. centres
def centre_groups(emim):
    """Groups of 1, 3, 64, 65 and 130 atoms of emim-BCN4: one lane, part of a wavefront, a full one, one past it, two passes.  Atom 100
    is in two groups; masses as weights, and explicit weights with one zero among them."""
    rng = np.random.default_rng(4)
    w65 = rng.uniform(0.5, 20.0, 65)
    w65[7] = 0.0
    return [(np.array([40]), None), (np.array([100, 101, 102]), None), (np.arange(200, 264), list(rng.uniform(1.0, 16.0, 64))),
            (np.concatenate([[100], np.arange(300, 364)]), list(w65)), (np.arange(500, 630), None)]


def test_centres_against_the_reference(emim):
    groups = centre_groups(emim)
    pos, masses, box = emim['positions'], emim['mass'], emim['box']
    n = len(pos)
    # distance(g1, g2): group 1 (three atoms) is in two bonds, group 3 holds an atom of group 1
    rows, par = [[0, 1], [2, 3], [1, 2]], [[300.0, 0.5], [250.0, 0.4], [200.0, 0.6]]
    for periodic in (False, True):
        L = box if periodic else None
        e, f, context = one_force(masses, box, centroid_force('centre-distance', groups, rows, par, periodic), pos)
        members = [with_groups(r, groups, masses) for r in rows]
        assert all(C.usable(C.TEXTS['centre-distance'], pos, m, p, L) for m, p in zip(members, par))
        e_ref, f_ref = C.total(*C.bond_sum(C.TEXTS['centre-distance'], members, par, pos, L), n)
        assert_close(e, f, e_ref, f_ref, 'emim / distance(g1,g2) over groups of 1, 3, 64, 65 atoms, periodic %s' % periodic)
        assert not f[300 + 7 - 1].any() and f[300].any()          # the member of weight zero feels nothing
    rows, par = [[0, 1, 2], [3, 2, 1]], [[40.0, 1.8], [30.0, 2.0]]
    e, f, _ = one_force(masses, box, centroid_force('centre-angle', groups, rows, par, True), pos)
    members = [with_groups(r, groups, masses) for r in rows]
    assert all(C.usable(C.TEXTS['centre-angle'], pos, m, p, box) for m, p in zip(members, par))
    e_ref, f_ref = C.total(*C.bond_sum(C.TEXTS['centre-angle'], members, par, pos, box), n)
    assert_close(e, f, e_ref, f_ref, 'emim / angle(g1,g2,g3) and x1 - x3 over centres')


def test_a_group_of_130_atoms(emim):
    """Two passes of the centre kernel: the centre through getCollectiveVariableValues of a CustomCVForce('x1'), the forces as w_i / W
    times the reference force on the centre."""
    groups = centre_groups(emim)
    pos, masses, box = emim['positions'], emim['mass'], emim['box']
    atoms = groups[4][0]
    with mpmath.workdps(R.DIGITS):
        W = mpmath.fsum(mpmath.mpf(float(m)) for m in masses[atoms])
        exact = [mpmath.fsum(mpmath.mpf(float(masses[a])) * mpmath.mpf(float(pos[a][c])) for a in atoms) / W for c in range(3)]
        exact_w = [float(mpmath.mpf(float(masses[a])) / W) for a in atoms]
    for c, axis in enumerate('xyz'):
        inner = openmm.CustomCentroidBondForce(1, axis + '1')
        inner.addGroup([int(a) for a in atoms])
        inner.addBond([0])
        cv = openmm.CustomCVForce('v')
        cv.addCollectiveVariable('v', inner)
        system = bare_system(masses, box)
        system.addForce(cv)
        context = context_with(system, pos)
        (got,) = cv.getCollectiveVariableValues(context)
        print('centre of 130 atoms, %s: %.17g (50 digits: %.17g, rel %.2e)' % (axis, got, float(exact[c]), abs(got - float(exact[c])) / abs(float(exact[c]))))
        assert abs(got - float(exact[c])) <= D_REL * abs(float(exact[c]))
    # the bond between this group and the three-atom group: the reference with the big group as ONE particle at the exact centre
    e, f, _ = one_force(masses, box, centroid_force('centre-distance', groups, [[4, 1]], [[300.0, 0.5]]), pos)
    extended = np.concatenate([pos, [[float(c) for c in exact]]])
    small = with_groups([1], groups, masses)[0]
    energies, forces = C.bond_sum(C.TEXTS['centre-distance'], [[len(pos), small]], [[300.0, 0.5]], extended)
    on_centre = forces[0][len(pos)]
    f_ref = np.zeros_like(pos)
    f_ref[atoms] = np.array(exact_w)[:, None] * on_centre
    for a in small[0]:
        f_ref[a] = forces[0][a]
    assert_close(e, f, float(energies[0]), f_ref, 'emim / distance between a group of 130 atoms and one of 3')


def test_single_atom_groups_are_the_compound_bond(emim):
    bonds, par = emim['bonds'][:300], harmonic_rows(emim)['harmonic-bond'][1][:300]
    atoms = sorted({int(a) for a in bonds.ravel()})
    where = {a: k for k, a in enumerate(atoms)}
    groups = [(np.array([a]), [1.0]) for a in atoms]
    force = openmm.CustomCentroidBondForce(2, C.TEXTS['harmonic-bond']['text'].replace('p', 'g'))
    for name in C.TEXTS['harmonic-bond']['names']:
        force.addPerBondParameter(name)
    for a, w in groups:
        force.addGroup([int(a[0])], w)
    for (i, j), row in zip(bonds, par):
        force.addBond([where[int(i)], where[int(j)]], [float(v) for v in row])
    e_c, f_c, _ = one_force(emim['mass'], emim['box'], force, emim['positions'])
    e_p, f_p, _ = one_force(emim['mass'], emim['box'], compound_force('harmonic-bond', bonds, par), emim['positions'])
    assert_close(e_c, f_c, e_p, f_p, 'emim / 300 bonds between single-atom groups of weight 1 against the compound bond')
    print('single-atom groups: energy bits equal %s, force bits equal %s' % (e_c == e_p, np.array_equal(f_c, f_p)))


# ------------------------------------------------------------------------------------ 6. determinism
def test_two_evaluations_and_the_two_instantiations_give_the_same_bits(emim):
    rows, params, _ = C.fixture_rows('sixteen', emim, 65)
    compound = compound_force('sixteen', rows, params, periodic=True)
    groups = centre_groups(emim)
    centroid = centroid_force('centre-angle', groups, [[0, 1, 2], [3, 2, 1], [4, 3, 0]], [[40.0, 1.8], [30.0, 2.0], [20.0, 1.5]], True)
    for force in (compound, centroid):
        _, _, context = one_force(emim['mass'], emim['box'], force, emim['positions'])
        ctx, fid = context._engine.ctx, context._engine.entries[0].term_ids[0]
        e, f = evaluate(ctx, fid, emim['positions'])
        again = evaluate(ctx, fid, emim['positions'])
        _, f_only = evaluate(ctx, fid, emim['positions'], energy=False)
        assert again[0] == e and np.array_equal(again[1], f) and np.array_equal(f_only, f) and np.abs(f).max() > 1.0
        # accumulate adds to what is there
        _, f_acc = evaluate(ctx, fid, emim['positions'], accumulate=True, start=np.ones_like(f))
        assert np.array_equal(f_acc, 1.0 + f)
        ctx.check()


# ------------------------------------------------------------------------------------ 7. as collective variables
def restraint_over(inner, K, d0):
    cv = openmm.CustomCVForce('0.5*K*(d-d0)^2')
    cv.addGlobalParameter('K', K)
    cv.addGlobalParameter('d0', d0)
    cv.addCollectiveVariable('d', inner)
    return cv


def test_a_centroid_distance_as_a_collective_variable(phenol):
    residue = phenol['residue']
    first, second = np.nonzero(residue == residue[0])[0], np.nonzero(residue == residue[-1])[0]
    assert len(first) == 13 and len(second) == 3
    masses, pos, box = phenol['mass'], phenol['positions'], phenol['box']

    def inner(text):
        force = openmm.CustomCentroidBondForce(2, text)
        force.addGroup([int(a) for a in first])
        force.addGroup([int(a) for a in second])
        force.addBond([0, 1])
        force.setUsesPeriodicBoundaryConditions(True)
        return force
    cv = restraint_over(inner('distance(g1,g2)'), 80.0, 0.9)
    direct = inner('0.5*K*(distance(g1,g2)-d0)^2')
    direct.addGlobalParameter('K', 80.0)
    direct.addGlobalParameter('d0', 0.9)
    e, f, context = one_force(masses, box, cv, pos)
    e_d, f_d, context_d = one_force(masses, box, direct, pos)
    assert_close(e, f, e_d, f_d, 'phenol / CustomCVForce over a centroid distance against the direct text')
    d = C.centre(pos, first, masses[first]) - C.centre(pos, second, masses[second])
    d -= box * np.rint(d / box)
    (got,) = cv.getCollectiveVariableValues(context)
    print('distance between the centres of mass: %.15g (numpy %.15g)' % (got, np.linalg.norm(d)))
    assert abs(got - np.linalg.norm(d)) <= D_REL * np.linalg.norm(d) and e == pytest.approx(40.0 * (got - 0.9) ** 2, rel=E_REL)
    for c in (context, context_d):
        c.setParameter('d0', 1.3)
    e2, f2 = energy_forces(context)
    assert_close(e2, f2, *energy_forces(context_d), 'phenol / the same after setParameter(d0)')
    assert e2 == pytest.approx(40.0 * (got - 1.3) ** 2, rel=E_REL) and e2 != e


def test_a_compound_dihedral_as_a_collective_variable(heaq):
    members = [int(a) for a in heaq['torsions'][0]]
    masses, pos, box = heaq['mass'], heaq['positions'], heaq['box']

    def inner(text):
        force = openmm.CustomCompoundBondForce(4, text)
        force.addBond(members)
        return force
    cv = restraint_over(inner('dihedral(p1,p2,p3,p4)'), 60.0, 0.5)
    direct = inner('0.5*K*(dihedral(p1,p2,p3,p4)-d0)^2')
    direct.addGlobalParameter('K', 60.0)
    direct.addGlobalParameter('d0', 0.5)
    e, f, context = one_force(masses, box, cv, pos)
    e_d, f_d, context_d = one_force(masses, box, direct, pos)
    assert_close(e, f, e_d, f_d, 'HEAQ / CustomCVForce over a compound dihedral against the direct text')
    case = dict(text='dihedral(p1,p2,p3,p4)', names=[], globals={})
    phi = float(C.exact_bond(case, pos, members, [], forces=False)[0])
    (got,) = cv.getCollectiveVariableValues(context)
    print('dihedral of the solute: %.15g (50 digits %.15g)' % (got, phi))
    assert abs(got - phi) <= D_REL * abs(phi)
    for c in (context, context_d):
        c.setParameter('d0', -0.7)
    e2, f2 = energy_forces(context)
    assert_close(e2, f2, *energy_forces(context_d), 'HEAQ / the same after setParameter(d0)')
    assert e2 == pytest.approx(30.0 * (got + 0.7) ** 2, rel=E_REL)


# ------------------------------------------------------------------------------------ 8. running
def with_compound_texts(system, data, kinds):
    rows = harmonic_rows(data)
    classes = {'harmonic-bond': openmm.HarmonicBondForce, 'harmonic-angle': openmm.HarmonicAngleForce}
    for k, force in enumerate(list(system._forces)):
        for name in kinds:
            if type(force) is classes[name]:
                idx, params = rows[name]
                system._forces[k] = compound_force(name, idx, params, force.usesPeriodicBoundaryConditions(), force.getForceGroup())
    return system


def thermal_velocities(data, seed=2026):
    kT = unit.MOLAR_GAS_CONSTANT_R._value * 300.0
    return np.random.default_rng(seed).normal(size=data['positions'].shape) * np.sqrt(kT / data['mass'])[:, None]


def test_twenty_verlet_steps_with_compound_bond_and_angle_texts(spcfw):
    xs = []
    for custom in (False, True):
        system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
        if custom:
            with_compound_texts(system, spcfw, ('harmonic-bond', 'harmonic-angle'))
        integrator = openmm.VerletIntegrator(0.001)
        context = context_with(system, spcfw['positions'], integrator)
        context.setVelocities(thermal_velocities(spcfw))
        assert sum(getattr(e, 'compound', None) is not None for e in context._engine.entries) == (2 if custom else 0)
        integrator.step(20)
        xs.append(positions_of(context))
        context._engine.ctx.check()
    worst, moved = np.abs(xs[0] - xs[1]).max(), np.abs(xs[0] - spcfw['positions']).max()
    print('20 Verlet steps, compound bond and angle texts against the harmonic kinds: max |dx| = %.3e nm, atoms moved up to %.3e nm' % (worst, moved))
    assert moved > 1e-3 and worst <= X_ABS


def test_four_respa_steps_fusion_on_and_off(spcfw):
    """Compound bond and angle texts in group 0 of RESPA [4, 2, 1]: the fusion rules decline the group, it is evaluated member by
    member (0 epilogue launches), and the steps end at the same bits with fusion on and off."""
    results = []
    for fuse in (True, False):
        system = with_compound_texts(system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic'), spcfw, ('harmonic-bond', 'harmonic-angle'))
        system = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
        context = context_with(system, spcfw['positions'], integrator)
        context.setVelocities(thermal_velocities(spcfw))
        context._engine.ctx.set_fuse_inner(fuse)
        assert [(type(e.force).__name__, e.group) for e in context._engine.entries if getattr(e, 'compound', None)] == [('CustomCompoundBondForce', 0)] * 2
        integrator.step(4)
        results.append((positions_of(context), context._engine.ctx.run_stats()))
        context._engine.ctx.check()
    (x_on, stats_on), (x_off, stats_off) = results
    print('4 RESPA [4, 2, 1] steps: run statistics with fusion %s, without %s' % (stats_on, stats_off))
    assert np.array_equal(x_on, x_off) and stats_on['epilogues'] == 0 and stats_off['epilogues'] == 0
    assert np.abs(x_on - spcfw['positions']).max() > 1e-4


def two_molecules():
    """Two bent triatomic molecules 0.9 nm apart, harmonic bonds and angles inside each."""
    one = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.13, 0.095, 0.0]])
    pos = np.concatenate([one + [1.0, 1.0, 1.0], one[:, [1, 0, 2]] + [1.9, 1.1, 1.05]])
    bonds, angles = openmm.HarmonicBondForce(), openmm.HarmonicAngleForce()
    for base in (0, 3):
        bonds.addBond(base, base + 1, 0.1, 2.0e5)
        bonds.addBond(base + 1, base + 2, 0.1, 2.0e5)
        angles.addAngle(base, base + 1, base + 2, 1.9, 400.0)
    return pos, [16.0, 12.0, 1.0] * 2, bonds, angles


def test_minimisation_pulls_a_centroid_distance_to_its_restraint():
    pos, masses, bonds, angles = two_molecules()
    k, d0 = 1000.0, 0.6
    groups = [(np.arange(0, 3), None), (np.arange(3, 6), None)]
    force = centroid_force('centre-distance', groups, [[0, 1]], [[k, d0]])
    system = bare_system(masses, BOX)
    for f in (bonds, angles, force):
        system.addForce(f)
    sim = app.Simulation(app.Topology(6), system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'))
    sim.context.setPositions(pos * unit.nanometers)
    e0 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    sim.minimizeEnergy()
    e1 = sim.context.getState(getEnergy=True).getPotentialEnergy()._value
    x = positions_of(sim.context)
    m = np.array(masses)
    before = np.linalg.norm(C.centre(pos, range(3), m[:3]) - C.centre(pos, range(3, 6), m[3:]))
    after = np.linalg.norm(C.centre(x, range(3), m[:3]) - C.centre(x, range(3, 6), m[3:]))
    width = math.sqrt(2.494339 / k)         # kT at 300 K over the restraint's constant: its thermal width
    print('minimisation: E %.6g -> %.6g kJ/mol, distance between the centres %.4f -> %.4f (d0 %.4f, thermal width %.4f)' % (e0, e1, before, after, d0, width))
    assert e1 < e0 and abs(before - d0) > 4 * width and abs(after - d0) < width
    sim.context._engine.ctx.check()


def test_langevin_middle_with_a_barostat(phenol):
    residue = phenol['residue']
    first, second = np.nonzero(residue == residue[0])[0], np.nonzero(residue == residue[-1])[0]
    system = system_from_arrays(phenol, nonbondedMethod='CutoffPeriodic', cutoff=0.9)
    groups = [(first, None), (second, None)]
    system.addForce(centroid_force('centre-distance', groups, [[0, 1]], [[100.0, 0.8]], periodic=True))
    system.addForce(compound_force('urey-bradley', phenol['angles'][:8], [[1.9, 50.0, 0.2, 500.0]] * 8, periodic=True))
    barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, 10)
    barostat.setRandomNumberSeed(11)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(300 * unit.kelvin, 1 / unit.picosecond, 1 * unit.femtoseconds)
    integrator.setRandomNumberSeed(3)
    context = context_with(system, phenol['positions'], integrator)
    context.setVelocitiesToTemperature(300.0, 5)
    energies = []
    for _ in range(5):
        integrator.step(10)
        energies.append(context.getState(getEnergy=True).getPotentialEnergy()._value)
    stats = context._engine.barostat_stats
    print('LangevinMiddle + barostat, 50 steps: %s; potential energies %s' % (stats, ['%.6g' % e for e in energies]))
    assert stats['attempts'] == 5 and all(math.isfinite(e) for e in energies) and np.isfinite(positions_of(context)).all()
    context._engine.ctx.check()


def test_free_space_system_with_a_centroid_restraint():
    pos, masses, bonds, angles = two_molecules()
    system = bare_system(masses)
    nb = openmm.NonbondedForce()
    for _ in range(6):
        nb.addParticle(0.0, 0.3, 0.0)
    nb.setNonbondedMethod(nb.NoCutoff)
    groups = [(np.arange(0, 3), None), (np.arange(3, 6), [1.0, 1.0, 2.0])]
    force = centroid_force('centre-distance', groups, [[0, 1]], [[300.0, 0.6]])
    for f in (nb, bonds, angles, force):
        f.setForceGroup(0 if f is not force else 1)
        system.addForce(f)
    integrator = openmm.VerletIntegrator(0.001)
    context = context_with(system, pos, integrator)
    assert context._engine.free_space
    e, f = energy_forces(context, groups={1})
    m = np.array(masses)
    c1, c2 = C.centre(pos, range(3), m[:3]), C.centre(pos, range(3, 6), [1.0, 1.0, 2.0])
    d = np.linalg.norm(c1 - c2)
    assert e == pytest.approx(150.0 * (d - 0.6) ** 2, rel=E_REL)
    assert np.allclose(f[:3], (m[:3] / m[:3].sum())[:, None] * (-300.0 * (d - 0.6) * (c1 - c2) / d), rtol=1e-9, atol=0.0)
    integrator.step(10)
    assert np.isfinite(positions_of(context)).all() and np.abs(positions_of(context) - pos).max() > 1e-5
    periodic = centroid_force('centre-distance', groups, [[0, 1]], [[300.0, 0.6]], periodic=True)
    system.addForce(periodic)
    with pytest.raises(atomsmm.InputError, match='periodic boundary'):
        openmm.Context(system, openmm.VerletIntegrator(0.001))
    context._engine.ctx.check()


# ------------------------------------------------------------------------------------ 9. refusals at the C-ABI
def test_abi_refusals_name_the_cause():
    n = 6
    pos, _, _, _ = two_molecules()
    prog, table = X.compile_compound('distance(p1,p2)', 2, 'p', [], [])
    kinds, slots = [B.CVAR_DISTANCE], [[0, 1]]
    ctx = B.HipContext(n, BOX)
    nobox = B.HipContext(n, None)
    try:
        def create(c=ctx, n_slots=2, kinds=kinds, slots=slots, idx=((0, 1),), params=np.zeros((0, 1)), periodic=False, groups=None, prog=prog):
            return c.compound_create(n_slots, prog.code, prog.consts, [], kinds, slots, np.array(idx, dtype=np.int32), params, periodic=periodic, groups=groups)
        with pytest.raises(B.HipError, match=r'amm_compound_create: 9 particles \(or groups\) per bond \(1 \.\. 8\)'):
            create(n_slots=9, idx=(tuple(range(6)) + (0, 1, 2),))
        with pytest.raises(B.HipError, match=r'amm_compound_create: 17 geometric variables \(limit 16\)'):
            create(kinds=kinds * 17, slots=slots * 17)
        with pytest.raises(B.HipError, match=r'amm_compound_create: 9 per-bond parameters \(limit 8\)'):
            create(params=np.zeros((9, 1)))
        with pytest.raises(B.HipError, match='amm_compound_create: atom index 6 of bond 0 is out of range'):
            create(idx=((0, 6),))
        with pytest.raises(B.HipError, match='amm_compound_create: atom index -1 of bond 1 is out of range'):
            create(idx=((0, 1), (-1, 2)))
        with pytest.raises(B.HipError, match=r'amm_compound_create: variable 0 names slot 2 beyond the bond \(2 slots\)'):
            create(slots=[[0, 2]])
        with pytest.raises(B.HipError, match='amm_compound_create: variable 0 has the unknown kind 6'):
            create(kinds=[6])
        with pytest.raises(B.HipError, match='amm_compound_create: periodic bonds, but the context has no periodic box'):
            create(c=nobox, periodic=True)
        two = X.compile_compound('distance(p1,p2)*x1', 2, 'p', [], [])[0]
        with pytest.raises(B.HipError, match=r'amm_compound_create: variable index out of range \(the kind has 1\)'):
            create(prog=two)
        with_p = X.compile_compound('k*distance(p1,p2)', 2, 'p', ['k'], [])[0]
        with pytest.raises(B.HipError, match=r'amm_compound_create: per-term parameter index out of range \(the force has 0\)'):
            create(prog=with_p)
        ptr, atoms = np.array([0, 3, 6], dtype=np.int32), np.arange(6, dtype=np.int32)
        with pytest.raises(B.HipError, match='amm_compound_create: group index 2 of bond 0 is out of range'):
            create(idx=((0, 2),), groups=(ptr, atoms, np.ones(6)))
        with pytest.raises(B.HipError, match='amm_compound_create: the weights of group 1 sum to'):
            create(groups=(ptr, atoms, np.array([1.0, 1.0, 1.0, 1.0, -2.0, 1.0])))
        with pytest.raises(B.HipError, match='amm_compound_create: group 1 is empty'):
            create(groups=(np.array([0, 6, 6], dtype=np.int32), atoms, np.ones(6)))
        with pytest.raises(B.HipError, match='amm_compound_create: atom index 6 of a group is out of range'):
            create(groups=(ptr, np.array([0, 1, 2, 3, 4, 6], dtype=np.int32), np.ones(6)))
        fid = create()
        centroid = create(groups=(ptr, atoms, np.ones(6)))
        e, f = evaluate(ctx, fid, pos)
        assert e == pytest.approx(0.1, rel=1e-12) and f[0, 0] == pytest.approx(1.0, rel=1e-12) and not f[2:].any()
        e, f = evaluate(ctx, centroid, pos)
        assert e == pytest.approx(np.linalg.norm(pos[:3].mean(axis=0) - pos[3:].mean(axis=0)), rel=1e-12) and np.abs(f.sum(axis=0)).max() < 1e-12
        # the other families refuse the id, naming the type
        for call in (lambda: ctx.bonded_add_terms(fid, B.BOND_HARMONIC, [[0, 1]], [[0.1, 1.0]]), lambda: ctx.bonded_finalize(fid),
                     lambda: ctx.bonded_release(fid), lambda: ctx.term_expr_set_globals(fid, []), lambda: ctx.term_expr_release(fid),
                     lambda: ctx.term_expr_set_params(fid, np.zeros((0, 1)), 1), lambda: ctx.pair_set_params(fid, np.zeros(n), np.zeros(n), np.zeros(n)),
                     lambda: ctx.pme_set_charges(fid, np.zeros(n))):
            with pytest.raises(B.HipError, match='AMM_FORCE_COMPOUND'):
                call()
        with pytest.raises(B.HipError, match='amm_compound_set_globals: the program reads 0 globals, 1 given'):
            ctx.compound_set_globals(fid, [1.0])
        with pytest.raises(B.HipError, match='amm_compound_set_params: the force has 1 bonds of 0 parameters, 1 x 2 given'):
            ctx.compound_set_params(fid, np.zeros((2, 1)), 1)
        with pytest.raises(B.HipError, match='amm_compound_set_weights: the force has no groups'):
            ctx.compound_set_weights(fid, np.ones(6))
        with pytest.raises(B.HipError, match='amm_compound_set_weights: the groups have 6 members, 5 weights given'):
            ctx.compound_set_weights(centroid, np.ones(5))
        with pytest.raises(B.HipError, match='amm_compound_set_weights: the weights of group 0 sum to'):
            ctx.compound_set_weights(centroid, np.array([1.0, -1.0, 0.0, 1.0, 1.0, 1.0]))
        ctx.compound_set_weights(centroid, np.array([1.0, 0.0, 0.0, 1.0, 1.0, 1.0]))
        e, f = evaluate(ctx, centroid, pos)
        assert e == pytest.approx(np.linalg.norm(pos[0] - pos[3:].mean(axis=0)), rel=1e-12) and not f[1:3].any()
        # a released inner id under a collective-variable force: refused before anything launches, the buffer keeps what it held
        outer = X.compile_cv('2*cv1', ['cv1'], [], [])
        cv = ctx.cv_create([fid], 0, outer.code, outer.consts, [])
        e2, f2 = evaluate(ctx, cv, pos)
        assert e2 == pytest.approx(0.2, rel=1e-12) and f2[0, 0] == pytest.approx(2.0, rel=1e-12)
        ctx.compound_release(fid)
        start = np.full((n, 3), 7.0)
        held = dev(start)
        with pytest.raises(B.HipError, match=r'inner force 0 \(id %d\) is a released id' % fid):
            ctx.force_eval(cv, dev(pos), held, accumulate=False, energy=None)
        ctx.synchronize()
        assert np.array_equal(held.cpu().numpy(), start)
        with pytest.raises(B.HipError, match='amm_compound_release: not the id of a compound-bond force'):
            ctx.compound_release(fid)
        with pytest.raises(B.HipError, match='released force id'):
            evaluate(ctx, fid, pos)
        ctx.check()
    finally:
        ctx.close()
        nobox.close()
