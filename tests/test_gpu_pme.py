"""GPU tests of the PME reciprocal space (csrc/pme.hip) through the C-ABI: energy and FORCES against the same algorithm on the same
mesh in plain numpy (tests/pme_cases.py, itself checked by tests/test_pme_host.py), on every way the kernels have of building the
charge mesh -- device atomics, tiles binned through LDS counters, tiles binned through global counters, the long scan, the
two-level ticket -- and through re-arming, two forces in one context, accumulation, new charges, a new box and the sliced gather.

Tolerances come from the reference alone (pme_cases.tolerances): with F, E the exact reference and F_q, E_q the one whose spread
contributions are rounded to multiples of 2^-42 as the kernels round theirs, dF = max|F_q - F|, dE = |E_q - E|,

    max|F_gpu - F| <= 4 dF + 256 eps max|F|,      |E_gpu - E| <= 4 dE + 256 eps (E_rec + |E_self|),      dF >= 1e-14 max|F|.

dF is about 1e-12 of max|F|: the check is six orders tighter than the comparison with an explicit Ewald sum can be.  Every
comparison also prints the distance to the QUANTISED reference (expected near 1e-15; DESIGN.md section 4 records what was
measured) -- information, not an assertion."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import pme_cases as PC  # noqa: E402

EPS = np.finfo(np.float64).eps


def dev(a):
    return torch.tensor(np.array(a, dtype=np.float64), device='cuda')        # (a copy: the cases' arrays are read-only)


@contextlib.contextmanager
def context(n, box, **kw):
    from atomsmm_amd import backend as B
    ctx = B.HipContext(n, box, **kw)
    try:
        yield ctx
    finally:
        ctx.close()


def evaluate(ctx, fid, pos, n):
    """As a group evaluation does: the force buffer holds NaN before, the energy scalar zero."""
    f = torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')
    en = torch.zeros(1, dtype=torch.float64, device='cuda')
    ctx.force_eval(fid, dev(pos), f, accumulate=False, energy=en)
    ctx.check()
    return en.item(), f.cpu().numpy()


def compare(label, e, f, t, q):
    """One evaluation (e, f) against the reference t = pme_cases.tolerances(...) of the same positions, box and charges q."""
    print('%s: vs exact dF/max|F| %.2e dE/|E| %.2e | vs quantised dF/max|F| %.2e dE/|E| %.2e | reference dF/max|F| %.2e dE/|E| %.2e'
          % (label, np.abs(f - t['F']).max() / t['fmax'], abs(e - t['E']) / abs(t['E']), np.abs(f - t['F_q']).max() / t['fmax'],
             abs(e - t['E_q']) / abs(t['E']), t['dF'] / t['fmax'], t['dE'] / abs(t['E'])))
    assert not np.isnan(f).any()
    assert (f[np.asarray(q) == 0] == 0.0).all()
    assert np.abs(f - t['F']).max() <= t['tol_F']
    assert abs(e - t['E']) <= t['tol_E']


def tolerances(c, pos=None, box=None, q=None):
    return PC.tolerances(c['pos'] if pos is None else pos, c['box'] if box is None else box, c['q'] if q is None else q,
                         c['alpha'], c['K'], c['Kc'])


@pytest.mark.parametrize('name', PC.CASES)
def test_forces_and_energy_vs_same_mesh_reference(name):
    """All seven meshes of pme_cases.MESHES: no NaN left of the buffer's, exact zeros on atoms without charge, energy and forces
    within the derived tolerance, the quantisation term of the tolerance alive, and a second evaluation bit for bit the first."""
    c = PC.case(name)
    t = PC.case_tolerances(name)
    n = len(c['q'])
    assert t['dF'] >= 1e-14 * t['fmax']
    with context(n, c['box']) as ctx:
        fid = ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])
        e, f = evaluate(ctx, fid, c['pos'], n)
        compare(name, e, f, t, c['q'])
        e2, f2 = evaluate(ctx, fid, c['pos'], n)
        assert e2 == e and np.array_equal(f2, f)


@pytest.mark.parametrize('name', ['ragged', 'global_bins'])
def test_one_force_rearms_between_different_position_sets(name):
    """Three position sets through ONE force object -- the case's, another seed's, and every atom inside a single tile (all other
    tiles empty) -- each against its reference, then the first again, bit for bit: no stale bin counter, ticket or stage tile."""
    c = PC.case(name)
    n = len(c['q'])
    sets = [('own', c['pos']), ('second seed', PC.case(name, 1)['pos']), ('one tile', PC.one_tile_positions(c))]
    with context(n, c['box']) as ctx:
        fid = ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])
        first = None
        for label, pos in sets:
            t = PC.case_tolerances(name) if label == 'own' else tolerances(c, pos=pos)
            e, f = evaluate(ctx, fid, pos, n)
            compare('%s, %s positions' % (name, label), e, f, t, c['q'])
            first = first or (e, f)
        e, f = evaluate(ctx, fid, c['pos'], n)
        assert e == first[0] and np.array_equal(f, first[1])


def test_two_meshes_in_one_context_do_not_share_state():
    """An atomic-spread mesh and a tiled one over the same atoms, evaluated in turn: each matches its own reference every time."""
    c, K_atomic = PC.case('ragged'), PC.MESHES['atomic']
    n = len(c['q'])
    t = {'ragged': PC.case_tolerances('ragged'), 'atomic': PC.tolerances(c['pos'], c['box'], c['q'], c['alpha'], K_atomic, c['Kc'])}
    with context(n, c['box']) as ctx:
        fid = {'atomic': ctx.pme_create(c['alpha'], K_atomic, c['q'], Kc=c['Kc']),
               'ragged': ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])}
        seen = {}
        for turn in range(2):
            for which in ('atomic', 'ragged'):
                e, f = evaluate(ctx, fid[which], c['pos'], n)
                compare('%s mesh over the atoms of ragged, turn %d' % (which, turn), e, f, t[which], c['q'])
                if which in seen:
                    assert e == seen[which][0] and np.array_equal(f, seen[which][1])
                seen[which] = (e, f)


def test_accumulate_adds_to_the_buffer_and_the_energy_adds_to_the_scalar():
    """accumulate=True, energy=None: buffer = what it held + F (256 eps of the magnitudes involved).  The energy output ADDS to the
    scalar (include/atomsmm_hip.h, amm_force_eval: "*d_energy += E"): a scalar that held 7.25 holds 7.25 + E."""
    c = PC.case('aligned')
    t = PC.case_tolerances('aligned')
    n = len(c['q'])
    with context(n, c['box']) as ctx:
        fid = ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])
        e, f = evaluate(ctx, fid, c['pos'], n)
        compare('aligned', e, f, t, c['q'])
        known = np.random.default_rng(5).uniform(-1.0, 1.0, (n, 3)) * t['fmax']
        buf = dev(known)
        ctx.force_eval(fid, dev(c['pos']), buf, accumulate=True, energy=None)
        ctx.check()
        assert np.abs(buf.cpu().numpy() - (known + f)).max() <= 256 * EPS * t['fmax']
        # forces alone, not accumulating: the numbers of the evaluation with energy
        g = torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')
        ctx.force_eval(fid, dev(c['pos']), g, accumulate=False, energy=None)
        ctx.check()
        assert np.array_equal(g.cpu().numpy(), f)
        en = torch.full((1,), 7.25, dtype=torch.float64, device='cuda')
        ctx.force_eval(fid, dev(c['pos']), g, accumulate=False, energy=en)
        ctx.check()
        assert abs(en.item() - 7.25 - t['E']) <= t['tol_E']
        assert abs((en.item() - 7.25) - e) <= 4 * EPS * (abs(e) + 7.25)


def test_set_charges_replaces_charges_and_self_energy():
    """A second charge set with other zero entries and another sum of squares: energy (the new self term in it) and forces are the
    reference's for the second set, and the atoms that lost their charge get exact zeros."""
    c = PC.case('one_tile_halo')
    n = len(c['q'])
    q2 = 1.5 * PC.charges(np.random.default_rng(11), n, zero_every=7, zero_from=3)
    assert ((c['q'] == 0) != (q2 == 0)).sum() > 20 and abs((q2 * q2).sum() / (c['q'] ** 2).sum() - 1) > 0.5
    with context(n, c['box']) as ctx:
        fid = ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])
        e, f = evaluate(ctx, fid, c['pos'], n)
        compare('one_tile_halo, first charges', e, f, PC.case_tolerances('one_tile_halo'), c['q'])
        ctx.pme_set_charges(fid, q2)
        e, f = evaluate(ctx, fid, c['pos'], n)
        compare('one_tile_halo, second charges', e, f, tolerances(c, q=q2), q2)


def test_box_change_against_the_reference_at_the_new_box():
    """amm_set_box with the mesh unchanged, three times by different factors, the positions scaled along: the absolute counterpart
    of the comparison with a fresh context in tests/test_gpu_box.py."""
    c = PC.case('ragged')
    n = len(c['q'])
    with context(n, c['box']) as ctx:
        fid = ctx.pme_create(c['alpha'], c['K'], c['q'], Kc=c['Kc'])
        e, f = evaluate(ctx, fid, c['pos'], n)
        compare('ragged, box as created', e, f, PC.case_tolerances('ragged'), c['q'])
        for scale in ((1.07, 1.07, 1.07), (0.93, 1.0, 1.12), (1.21, 0.88, 0.97)):
            s = np.array(scale)
            ctx.set_box(c['box'] * s)
            e, f = evaluate(ctx, fid, c['pos'] * s, n)
            compare('ragged, box scaled by %s' % (scale,), e, f, tolerances(c, pos=c['pos'] * s, box=c['box'] * s), c['q'])


@pytest.mark.parametrize('n, world', [(97, 3), (5, 8)])
def test_sliced_gather_without_a_communicator(n, world):
    """amm_pme_set_sliced on contexts that are rank r of `world` (no communicator: each is evaluated on its own), on the first n
    atoms of 'ragged'; n = 5 on 8 ranks leaves ranks 5 to 7 without an atom.  Rows of the rank's block [r ceil(n / world), ...) are
    the reference's; the others are exact zeros, or untouched when accumulating; the energy scalar gets the full energy on rank 0
    and is left alone elsewhere; the ranks' forces add up to the single-rank forces bit for bit."""
    c = PC.case('ragged')
    pos, q = c['pos'][:n], c['q'][:n]
    t = tolerances(c, pos=pos, q=q)
    with context(n, c['box']) as ctx:
        e1, f1 = evaluate(ctx, ctx.pme_create(c['alpha'], c['K'], q, Kc=c['Kc']), pos, n)
    compare('ragged[:%d], one rank' % n, e1, f1, t, q)
    per = -(-n // world)
    total = np.zeros((n, 3))
    for r in range(world):
        a0 = min(n, r * per)
        a1 = min(n, a0 + per)
        assert (a1 > a0) == (r < 5) or n != 5
        inside = np.zeros(n, dtype=bool)
        inside[a0:a1] = True
        with context(n, c['box'], rank=r, world=world) as ctx:
            fid = ctx.pme_create(c['alpha'], c['K'], q, Kc=c['Kc'])
            ctx.pme_set_sliced(fid)
            f = torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')
            en = torch.full((1,), 7.25, dtype=torch.float64, device='cuda')
            ctx.force_eval(fid, dev(pos), f, accumulate=False, energy=en)
            ctx.check()
            f = f.cpu().numpy()
            assert not np.isnan(f).any()
            assert (f[~inside] == 0.0).all()
            assert np.abs(f[inside] - t['F'][inside]).max(initial=0.0) <= t['tol_F']
            assert np.array_equal(f[inside], f1[inside])
            if r == 0:
                assert abs(en.item() - 7.25 - t['E']) <= t['tol_E']
            else:
                assert en.item() == 7.25
            total += f
            known = np.random.default_rng(r).uniform(-1.0, 1.0, (n, 3)) * t['fmax']
            buf = dev(known)
            ctx.force_eval(fid, dev(pos), buf, accumulate=True, energy=None)
            ctx.check()
            buf = buf.cpu().numpy()
            assert np.array_equal(buf[~inside], known[~inside])
            assert np.abs(buf[inside] - (known + f)[inside]).max(initial=0.0) <= 256 * EPS * t['fmax']
    assert np.array_equal(total, f1)
