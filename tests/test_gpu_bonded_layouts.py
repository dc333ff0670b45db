"""The bond-list kernels (csrc/bonded.hip, csrc/bonded_terms.h) on every device layout amm_bonded_finalize builds and every launch
the scheduler chooses from them, against an mpmath reference (tests/bonded_ref.py) on the topology zoo of tests/bonded_cases.py --
whose docstring lists the guards, the case on each, and the measured tolerances.  Everything goes through backend.HipContext.

  (a) record walk (k_bonded): energy and forces against the reference, in the units S_i / sum |E_t| at 16 x the measured fp64 loss;
      the layout the case was built for is asserted through amm_bonded_stats
  (b) term-parallel (k_terms_eval + k_terms_gather, option terms_from = 1), overwriting and accumulating onto ones: the bits of (a)
  (c) inner iterations through amm_run_ops: fused == plain bit for bit, the rule the layout admits, option no_term_lanes, one bathed
      run on Z6-8, rule 5 (E K K M) with terms_from = 1 and, where mixed_ok, the same bits with option mixed_terms = 0.  The plain run
      is also held against tests/ops_ref.py driven by the reference's forces where the program opens with the iteration (n = 1 and 3,
      both numberings) and in the rule-5 program; the pre-kicked programs are checked fused against plain only (their trajectories
      would need reference evaluations of their own: 0.1 .. 0.8 s each)
  (d) the molecule-row epilogue of the pair kernels in tip3p_box(8): three-site sets that ride on it and one near miss per condition
  (e) single terms at hard geometries: each within 32 x what a 1 ulp change of one input coordinate does to the force (+ 32 eps |F|);
      harmonic angles beyond their documented range: finite, and the energy within a derived bound

RESULTS (MI355X; the kernel takes theta = acos(c) and divides by sqrt(1 - c^2))
  (a) worst deviation from the reference over the 36 cases: 9.3e-14 S_i in the forces (Z9; bound 1.9e-12) and 6.7e-16 sum |E_t| in
      the energy (bound 1.2e-14); the fp64 restatement on the CPU loses 9.0e-14 and 5.5e-16.
  (c) against ops_ref over 108 comparisons: at most 4.4e-16 nm and 8.8e-14 nm/ps (bounds 1e-11, 1e-9).
  (e) harmonic angle at distance d from 0 or from pi; inside the range (d >= 1e-2) error / bound, beyond it the force's relative
      error (not asserted: include/atomsmm_hip.h documents the loss) and the asserted energy error / its bound:
          d                          1e-1   1e-2  |  1e-3             1e-4             1e-6             1e-8
          theta -> pi, theta0 = pi   0.00   0.00  |  0.00             0.00             0.00             0.00   (error / bound at every d: the
                                                                                                         force vanishes with d; asserted)
          theta -> pi, theta0 = 1.9  0.04   0.04  |  1e-10, E 0.07    2e-8, E 0.14     2e-4, E 0.10     0.33, E 0.08
          theta -> 0,  theta0 = pi   0.03   0.03  |  1e-10, E 0.06    3e-9, E 0.01     2e-4, E 0.10     1e4,  E 0.17
          theta -> 0,  theta0 = 1.9  0.03   0.03  |  1e-10, E 0.06    3e-9, E 0.01     2e-4, E 0.10     1e4,  E 0.17
      At d = 1e-3 the force is 2.1 x (towards pi) and 3.6 x (towards 0) its conditioning bound, at 1e-4 9 x and 44 x, below that up to 1e9 x; at
      1e-8 the angle is taken as exactly 0 or pi and the 1e-24 floor under 1 - c^2 sets the force.
      Bonds down to |r - r0| / r0 = 1e-15, torsions 1e-9 from phi = 0 and +-pi and with a triple 1e-3 from collinear: error / bound 0.00.
      A displacement 1 ulp above L/2: the kernel (d * (1/L), rounded) chooses the other image than d / L does; its force equals that
      image's to 0.06 of 32 eps (|F| + |dF/dr|).
  The whole module (300 tests) takes 31 s, the slowest test (three iterations against ops_ref on Z6-9) 1.0 s.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import bonded_cases as Z  # noqa: E402
import bonded_ref as R  # noqa: E402
import ops_ref  # noqa: E402
from ops_ref import CP, E, K, M  # noqa: E402
import test_gpu_op_programs as P  # noqa: E402  (Rig, execute, compare: the scheduler module's machinery; its tests are not re-collected)

FS = 0.001
H0, D0 = 0.125 * FS, 0.25 * FS
IT0 = [K(0, H0), M(D0), E(0), K(0, H0)]
IT0_BATH = [K(0, H0), M(0.5 * D0), (P.OP_BATH, 0, P.SLOT_V, 0, 0.0), M(0.5 * D0), E(0), K(0, H0)]
PRE = [K(3, 0.21 * FS), K(3, 0.09 * FS)]
WORST = {'force': 0.0, 'energy': 0.0}


def _B():
    from atomsmm_amd import backend as B
    return B


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def add_set(ctx, case):
    """the case's terms as one bond-list set, kind by kind"""
    B = _B()
    fid = ctx.bonded_create()
    near = B.pair_desc(B.NEAR_SHIFT, R.CONSTS['rc0'], rc0=R.CONSTS['rc0'], rs0=R.CONSTS['rs0'])
    ewald = B.pair_desc(B.NEAR_NONE, 1.0, alpha=R.CONSTS['alpha'], Kc=R.CONSTS['Kc'])
    for kind in range(8):
        idx, par = case.kind_arrays(kind)
        if len(idx):
            ctx.bonded_add_terms(fid, kind, idx, par, periodic=case.periodic[kind], desc={Z.NEAR: near, Z.EWALD: ewald}.get(kind))
    ctx.bonded_finalize(fid)
    return fid


def evaluate(case, terms_from=None, energy=True, accumulate_onto=None):
    """forces (and energy) of the case's set on a fresh context -> (forces [n][3], energy or None, stats)"""
    B = _B()
    ctx = B.HipContext(case.n, case.box)
    if terms_from is not None:
        ctx.set_option('terms_from', terms_from)
    fid = add_set(ctx, case)
    stats = ctx.bonded_stats(fid)
    x = dev(case.x)
    f = torch.full((case.n, 3), float('nan') if accumulate_onto is None else accumulate_onto, dtype=torch.float64, device='cuda')
    e = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, x, f, accumulate=accumulate_onto is not None, energy=e)
    ctx.check()
    out = f.cpu().numpy().copy(), (float(e.cpu()[0]) if energy else None), stats
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def record_walk(name):
    return evaluate(Z.zoo()[name])


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize('name', Z.ALL_NAMES)
def test_record_walk_against_reference(name):
    case, ref = Z.zoo()[name], Z.reference(name)
    f, e, stats = record_walk(name)
    assert stats == case.expect
    S = ref.units(case)
    # the restatement's part of kind k at an atom stays below W[k] S_i, so an atom is held to 16 x the sum of W over the kinds it
    # carries: an atom without a harmonic bond (whose r - r0 sets W[all]) gets the far smaller figure of its own kinds
    W = np.array(Z.W_FORCE_CPU[:8])
    bound = Z.MARGIN * S * sum(W[k] * (ref.units(case, k) > 0) for k in range(8))
    bound = np.minimum(bound, Z.FORCE_BOUND * S)
    err = np.linalg.norm(f - ref.forces, axis=1)
    live = S > 0
    rf = float((err[live] / S[live]).max()) if live.any() else 0.0
    nobond = live & (ref.units(case, Z.BOND) == 0)
    if nobond.any():
        print('%s: atoms without a bond: worst %.2e S_i, their bounds %.2e .. %.2e' % (name, float((err[nobond] / S[nobond]).max()),
              float((bound[nobond] / S[nobond]).min()), float((bound[nobond] / S[nobond]).max())))
    re_ = abs(e - ref.energy) / ref.e_unit if ref.e_unit > 0 else 0.0
    WORST['force'], WORST['energy'] = max(WORST['force'], rf), max(WORST['energy'], re_)
    print('%s: force %.2e S_i (bound %.2e), energy %.2e sum|E_t| (bound %.2e); worst so far %.2e, %.2e'
          % (name, rf, Z.FORCE_BOUND, re_, Z.ENERGY_BOUND, WORST['force'], WORST['energy']))
    assert np.isfinite(f).all() and np.isfinite(e)
    assert (f[~live] == 0.0).all(), 'an atom without records got a force'
    assert (err <= bound).all(), 'worst %.3e S_i; atom %d has %.3e of a bound of %.3e' % (rf, int(np.argmax(err - bound)), err[int(np.argmax(err - bound))], bound[int(np.argmax(err - bound))])
    assert abs(e - ref.energy) <= Z.ENERGY_BOUND * ref.e_unit


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize('name', Z.ALL_NAMES)
def test_term_parallel_has_the_bits_of_the_record_walk(name):
    case = Z.zoo()[name]
    want = record_walk(name)[0]
    f, _, stats = evaluate(case, terms_from=1, energy=False)
    assert stats == case.expect_tf1
    assert np.array_equal(f, want), 'overwriting form'
    g, _, _ = evaluate(case, terms_from=1, energy=False, accumulate_onto=1.0)
    assert np.array_equal(g, 1.0 + want), 'accumulating form'


# ---------------------------------------------------------------------------------------------------------------- (c)
def reference_forces(case):
    """x -> the reference's forces (fp64 values of the mpmath sums) for ops_ref; the start geometry's are the cached ones"""
    import copy

    def forces(x):
        if np.array_equal(x, case.x):
            return Z.reference(case.name).forces
        moved = copy.copy(case)
        moved.x = np.ascontiguousarray(x)
        return R.Reference(moved).forces
    return forces


@functools.lru_cache(maxsize=None)
def rig(name, options=()):
    case = Z.zoo()[name]
    c = dict(positions=case.x, mass=case.mass, box=case.box)

    def define(ctx):
        ctx.group_define(0, 0, [add_set(ctx, case)])
        return []

    return P.Rig(name, c, case.v, (0, 3), [E(0), CP(3, 0)], define, {0: (0, [reference_forces(case)])}, options=options)


def expected_iterations(case, npre, n):
    """Rule 2 takes up to three pre-kicks and every iteration in one launch when max_comp <= 8.  Above that rule 3 takes one iteration
    per launch -- when the program opens with the iteration.  Behind pre-kicks op 0 is a KICK followed by a KICK, which rule 3 does
    not match, and rule 6 takes the pre-kicks, the iteration's opening KICK and its MOVE in one launch; EVAL is plain; the closing
    KICK is followed by the next iteration's opening KICK (again no rule 3) and goes to rule 6 with it and the MOVE; the program's
    last KICK is alone and plain: r6 = n, p = n + 1."""
    if case.expect['max_comp'] <= 8:
        return P.X(r2=1)
    return P.X(r3=n) if npre == 0 else P.X(r6=n, p=n + 1)


@pytest.mark.parametrize('npre,n', [(0, 1), (2, 1), (0, 3), (2, 3)])
@pytest.mark.parametrize('name', Z.ALL_NAMES)
def test_inner_iterations(name, npre, n):
    case = Z.zoo()[name]
    ops = PRE[:npre] + IT0 * n
    r = rig(name)
    # (the reference interpreter, driven by the mpmath forces, where the program opens with the iteration: one reference evaluation per
    # iteration, 0.1 .. 0.8 s each; the pre-kicked programs move along other trajectories and would double that)
    fused, plain = P.compare(r, ops, 1, ref=(npre == 0), label='%s pre%d x%d' % (name, npre, n))
    want = expected_iterations(case, npre, n)
    assert fused['counters'] == want, (fused['counters'], want)
    if case.expect['terms_ok']:
        other = P.execute(rig(name, (('no_term_lanes', 1),)), ops, 1, True)
        assert other['counters'] == fused['counters']
        for key in ('x', 'v'):
            assert np.array_equal(other[key], fused[key]), 'no_term_lanes changes %s' % key
        assert np.array_equal(other['bufs'][0], fused['bufs'][0])


@pytest.mark.parametrize('name', Z.ALL_NAMES)
def test_eval_kicks_move_with_term_tables(name):
    """option terms_from = 1: E K K M is one launch of rule 5 (k_mixed_eval_kicks where mixed_ok, k_terms_gather_kicks elsewhere); the
    iterations keep the rule of (c).  A set without terms has no term tables: rule 5 declines, the kicks and the move are rule 6."""
    case = Z.zoo()[name]
    r = rig(name, (('terms_from', 1),))
    ops = [E(0), K(0, 0.11 * FS), K(3, 0.13 * FS), M(0.5 * FS), E(0)]
    fused, _ = P.compare(r, ops, 1, label='%s EKKM' % name)
    assert fused['counters'] == (P.X(r5=1, p=1) if case.expect_tf1['n_gterms'] > 0 else P.X(p=2, r6=1))
    if case.expect_tf1['mixed_ok']:
        # option mixed_terms = 0 sends the same program through k_terms_eval + k_terms_gather_kicks: the same rule, the same bits -- and
        # a mixed launch that quietly fell back would make this comparison one of a path with itself, so the stats are asserted too
        other = P.execute(rig(name, (('terms_from', 1), ('mixed_terms', 0))), ops, 1, True)
        assert other['counters'] == fused['counters']
        for key in ('x', 'v'):
            assert np.array_equal(other[key], fused[key]), 'mixed launch and gather launch differ in %s' % key
        assert np.array_equal(other['bufs'][0], fused['bufs'][0])
    fused, _ = P.compare(r, IT0 * 3, 1, ref=False, label='%s x3, terms_from = 1' % name)
    assert fused['counters'] == expected_iterations(case, 0, 3)


def test_bathed_iterations_with_eight_term_lanes():
    """Z6-8 (G = 8 with term lanes) under an Ornstein-Uhlenbeck bath: K M BATH M E K iterations are one launch of rule 2"""
    for name in ('Z6-8', 'Z6-8~'):
        fused, _ = P.compare(rig(name), IT0_BATH * 3, 1, label='%s bathed' % name)
        assert fused['counters'] == P.X(r2=1)
        assert Z.zoo()[name].expect['terms_ok'] == 1 and Z.zoo()[name].expect['G'] == 8


# ---------------------------------------------------------------------------------------------------------------- (d)
def renumbered_water_box(variant):
    """tip3p_box(8) with every per-atom array and the exclusions renumbered: 'centre-slot-1' stores each molecule as H, O, H (Z2: the
    centre outside slot 0), 'interleaved' gives the first two waters the indices 0, 2, 4 and 1, 3, 5 (Z4), 'ion' appends one atom that
    no term and no pair force touches (zero charge and epsilon: Z4, 3 ncomp != n).  -> (arrays, new index of each old atom)"""
    from atomsmm_amd.testing import tip3p_box
    c = tip3p_box(8)
    n = len(c['positions'])
    new = np.arange(n)
    if variant == 'centre-slot-1':
        new = new + np.tile([1, -1, 0], n // 3)
    elif variant == 'interleaved':
        new[:6] = [0, 2, 4, 1, 3, 5]
    out = {}
    for key in ('positions', 'velocities', 'charge', 'sigma', 'epsilon', 'mass'):
        out[key] = np.empty_like(c[key])
        out[key][new] = c[key]
    for key in ('bonds', 'angles', 'exc_pairs'):
        out[key] = new[c[key]].astype(np.int32)
    out['exc_pairs'] = np.sort(out['exc_pairs'], axis=1)
    for key in ('box', 'bond_r0', 'bond_k', 'angle_theta0', 'angle_k'):
        out[key] = c[key]
    if variant == 'ion':
        out['positions'] = np.concatenate([out['positions'], [0.5 * c['box']]])
        out['velocities'] = np.concatenate([out['velocities'], [[0.1, -0.2, 0.3]]])
        for key, value in (('charge', 0.0), ('sigma', 1.0), ('epsilon', 0.0), ('mass', 22.99)):
            out[key] = np.append(out[key], value)
    return out


@functools.lru_cache(maxsize=None)
def water_rig(variant):
    """fixture W of test_gpu_op_programs (tip3p_box(8), near force-switch on the damped force's list) with another bond-list set"""
    from oracle import oracle as O
    B = _B()
    c = renumbered_water_box(variant)
    n = len(c['positions'])
    terms = [(Z.BOND, (int(i), int(j)), (r0, k)) for (i, j), r0, k in zip(c['bonds'], c['bond_r0'], c['bond_k'])]
    terms += [(Z.ANGLE, tuple(int(q) for q in a), (t0, k)) for a, t0, k in zip(c['angles'], c['angle_theta0'], c['angle_k'])]
    hh = 2 * c['bond_r0'][0] * np.sin(c['angle_theta0'][0] / 2)
    ends = [(int(a[0]), int(a[2])) for a in c['angles']]
    if variant in ('four-terms', 'five-terms', 'centre-slot-1'):
        terms += [(Z.BOND, e, (hh, 4.0e4)) for e in ends]
    if variant == 'five-terms':
        terms += [(Z.ANGLE, (int(a[1]), e[0], e[1]), (0.5 * (np.pi - c['angle_theta0'][0]), 100.0)) for a, e in zip(c['angles'], ends)]
    if variant == 'one-ljc':
        terms += [(Z.LJC, (4, 5), (0.17, 0.1, 0.2))]
    case = Z.Case('W-' + variant, n, c['box'], c['positions'], terms, (False,) * 8, {}, {})
    dn = O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5)
    dd = O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1)
    seen = {}

    def define(ctx):
        bid = add_set(ctx, case)
        seen['stats'] = ctx.bonded_stats(bid)
        nid, did = P._pair(B, ctx, dn, c), P._pair(B, ctx, dd, c)
        ctx.pair_share_list(nid, did)
        ctx.group_define(0, 0, [bid]); ctx.group_define(1, 1, [nid]); ctx.group_define(2, 2, [did])
        return [nid, did]

    r = P.Rig('W-' + variant, c, c['velocities'], (0, 1, 2, 3), [E(2), E(1), E(0), CP(3, 1)], define, None)
    r.seen, r.layout = seen, Z.layout(n, case.terms)
    return r


@pytest.mark.parametrize('variant,mol3', [('water', 1), ('four-terms', 1), ('centre-slot-1', 1), ('five-terms', 0), ('one-ljc', 0),
                                          ('interleaved', 0), ('ion', 0)])
def test_molecule_row_epilogue(variant, mol3):
    """The dual-plan program of test_gpu_op_programs (E(2) E(1), two pre-kicks, two inner iterations, E(1)).  Three-site sets with
    mol3_ok -- water's three terms (Z1); four terms == G with an H-H bond; the same with every molecule stored H, O, H, the centre in
    slot 1 (Z2) -- ride on the pair launch (epi = 1).  Each near miss turns the plan down (epi = 0, the iterations are rule 2): a fifth
    term (no term lanes), one BOND_LJC term, two waters whose indices interleave, one more atom without a term.  Fused == plain."""
    r = water_rig(variant)
    fused, _ = P.compare(r, [E(2), E(1)] + P.DUAL_TAIL, 1, ref=False, label='W-%s dual plan' % variant)
    assert r.seen['stats'] == r.layout and r.seen['stats']['mol3_ok'] == mol3
    assert fused['counters'] == (P.X(r4=1, off=1, epi=1, p=1) if mol3 else P.X(r4=1, r2=1, p=1))


# ---------------------------------------------------------------------------------------------------------------- (e)
EPS = 2.0 ** -52
HARD_DELTAS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-6, 1e-8)
ANGLE_RANGE = 1e-2          # include/atomsmm_hip.h: the harmonic angle's force is input-accurate while sin theta >= 1e-2
BOX3 = np.full(3, 3.0)


def _frame():
    u = np.array([0.36, 0.48, 0.8])
    w = np.cross(u, [0.0, 0.0, 1.0])
    w /= np.linalg.norm(w)
    return np.array([1.3, 0.9, 1.7]), u, w


def hard_terms():
    """{id: dict(kind, x [arity][3], p, and for angles delta, beyond)}: single terms at geometries where a formula can lose what the
    inputs still hold.  beyond: an angle closer to 0 or pi than the documented range whose force does not vanish there."""
    c0, u, w = _frame()
    out = {}
    for theta0, tag in ((np.pi, 'pi'), (1.9, '1.9')):
        for side in ('pi-', ''):
            for d in HARD_DELTAS:
                th = np.pi - d if side else d
                x = np.array([c0 + 0.12 * u, c0, c0 + 0.12 * (np.cos(th) * u + np.sin(th) * w)])
                harmless = theta0 == np.pi and side == 'pi-'          # F ~ k (pi - theta): the force vanishes with the distance
                out['angle-%s%g-theta0-%s' % (side, d, tag)] = dict(kind=Z.ANGLE, x=x, p=(theta0, 500.0), delta=d, theta=th,
                                                                   beyond=d < ANGLE_RANGE and not harmless)
    for rel in (1e-3, 1e-6, 1e-9, 1e-12, 1e-15):
        out['bond-%g' % rel] = dict(kind=Z.BOND, x=np.array([c0, c0 + 0.12 * (1.0 + rel) * u]), p=(0.12, 3.0e5))
    chain = [c0 + 0.12 * u, c0, c0 + 0.12 * (np.cos(1.9) * u + np.sin(1.9) * w)]
    for tag, phi in (('0+1e-9', 1e-9), ('pi-1e-9', np.pi - 1e-9), ('-pi+1e-9', -np.pi + 1e-9)):
        x = np.array(chain + [Z._place(chain[0], chain[1], chain[2], 0.12, 1.9, phi)])
        out['torsion-phi-%s' % tag] = dict(kind=Z.TORSION, x=x, p=(2.0, 1.1, 6.0))
    for d in (1e-2, 1e-3):
        x = np.array(chain + [Z._place(chain[0], chain[1], chain[2], 0.12, np.pi - d, 1.0)])
        out['torsion-triple-%g' % d] = dict(kind=Z.TORSION, x=x, p=(2.0, 1.1, 6.0))
    # |dF/dr| of the three pair kinds at r = L/2 (for the image test below): k, 2 k, and for the Ewald term a few |F| / r
    for kind, tag, p, stiff in ((Z.BOND, 'bond', (1.45, 500.0), 500.0), (Z.EWALD, 'ewald', (-0.35,), 100.0), (Z.VIR_H, 'virial', (1.4, 80.0), 160.0)):
        for side, towards in (('below', 0.0), ('above', 2.0)):
            out['half-box-%s-%s' % (tag, side)] = dict(kind=kind, x=np.array([[0.0, 2.9, 2.9], [np.nextafter(1.5, towards), 2.9, 2.9]]), p=p,
                                                       half_box=True, stiff=stiff)
    return out


HARD = hard_terms()


@functools.lru_cache(maxsize=None)
def hard_gpu(hid):
    """one hard term alone in Z9's box, by the record walk -> (forces [arity][3], energy)"""
    h = HARD[hid]
    case = Z.Case(hid, len(h['x']), BOX3, h['x'], [(h['kind'], tuple(range(len(h['x']))), h['p'])], Z.Z9_PERIODIC, {}, {})
    f, e, _ = evaluate(case)
    return f, e


def mp_forces(kind, x, p):
    e, f = R.term_forces_mp(kind, x, p, Z.Z9_PERIODIC[kind], BOX3)
    return float(e), np.array([[float(v) for v in row] for row in f])


def conditioning(kind, x, p):
    """(reference energy, forces, the largest change of any force component under a +-1 ulp change of one input coordinate)"""
    e0, f0 = mp_forces(kind, x, p)
    worst = 0.0
    for a in range(len(x)):
        for k in range(3):
            for towards in (-np.inf, np.inf):
                y = x.copy()
                y[a, k] = np.nextafter(y[a, k], towards)
                worst = max(worst, float(np.abs(mp_forces(kind, y, p)[1] - f0).max()))
    return e0, f0, worst


@pytest.mark.parametrize('hid', list(HARD))
def test_hard_geometry(hid):
    """Forces within 32 x what a 1 ulp change of one input coordinate does to them, + 32 eps |F|.

    Angles beyond the documented range of AMM_ANGLE_HARMONIC (closer than 1e-2 rad to 0 or pi, force not vanishing there): the kernel
    takes theta = acos(c) and divides by sqrt(1 - c^2), which the sweep showed to leave that bound from 1e-3 rad on (error / bound 2.1
    and 3.6 at 1e-3, 1e2 .. 1e9 below; near-linear angles through the cross product cured it but cost 0.3 % of the flagship step, so the
    kernel stayed).  There the test asserts finite forces and the energy: c carries at most dc = 8 eps of rounding (a dot product, two
    reciprocal square roots, two products), so theta is off by at most min(dc / sin theta, sqrt(2 dc)) -- the second when 1 - |c|
    itself is below dc and acos returns anything between 0 and acos(1 - dc) -- and E = k (theta - theta0)^2 / 2 by at most
    k (|theta - theta0| dtheta + dtheta^2 / 2) + 8 eps E.

    A displacement 1 ulp from L/2: either nearest image is a right answer (the force turns round between them, which is also what the
    conditioning bound says), so the result must equal the force of ONE of the two images, to 32 eps (|F| + |dF/dr|)."""
    h = HARD[hid]
    kind, x, p = h['kind'], h['x'], h['p']
    got, e_got = hard_gpu(hid)
    e_want, want, cond = conditioning(kind, x, p)
    fmax = float(np.abs(want).max())
    assert np.isfinite(got).all() and np.isfinite(e_got)
    if h.get('beyond'):
        dc = 8.0 * EPS
        dth = min(dc / np.sin(h['theta']), np.sqrt(2.0 * dc))
        e_bound = p[1] * (abs(h['theta'] - p[0]) * dth + 0.5 * dth * dth) + 8.0 * EPS * abs(e_want)
        print('%s (beyond the range): energy %.15e, error %.3e, bound %.3e; force error %.3e of |F| %.3e, inputs allow %.3e'
              % (hid, e_got, abs(e_got - e_want), e_bound, float(np.abs(got - want).max()), fmax, cond))
        assert abs(e_got - e_want) <= e_bound
        return
    if h.get('half_box'):
        other = want * np.array([-1.0, 1.0, 1.0])            # the displacement is along x: the other image turns that component round
        err = min(float(np.abs(got - want).max()), float(np.abs(got - other).max()))
        bound = 32.0 * EPS * (fmax + h['stiff'])
    else:
        err, bound = float(np.abs(got - want).max()), 32.0 * cond + 32.0 * EPS * fmax
    print('%s: |F| %.3e, error %.3e, inputs allow %.3e, bound %.3e (error / bound %.2f)' % (hid, fmax, err, cond, bound, err / bound if bound else np.inf))
    assert err <= bound
