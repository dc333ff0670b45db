"""The molecule-row pair kernels with site-site tables (csrc/cluster.hip: k_cpair / cwalk_rows) let a pair that does not count --
beyond the cutoff, a padding lane, below the table -- read a slot of zeros in LDS instead of throwing its force away by a select,
and no longer clamp the interval of a pair that counts.  Neither may change a bit, or the sign of a zero, of what the kernels
compute: forces of one evaluation and the state after 6 outer steps of RESPA [4, 2, 1] equal the goldens recorded by the build of
the commit before (scripts/record_zero_slot_goldens.py, kernel revision r08-buildtabs) -- array_equal and equal sign bits on the
atoms a golden keeps, the SHA-256 of the bytes of ALL atoms.

Cases (scripts/record_zero_slot_goldens.py: CASES), at the smallest boxes that reach each path: 1 536 atoms (3 cells per edge: the
per-pair-image loop) and 14 739 atoms (7 cells: interior and image/molecule tasks), each as the fused step-boundary pass and as two
launches of their own -- the near force has the same bits either way; a water whose oxygen sits at r^2 = rc^2 exactly and at the
last double below it from a partner's oxygen, for the near and for the outer cutoff; partners between rc and rc + skin beyond the
table's last interval; a pair pushed below the tables (the analytic redo) inside trips of ordinary pairs; molecules all of whose
listed partners are outside the cutoffs (their force is +0.0 in every component); rows whose length is no multiple of the lanes per
row; chargeless hydrogens (q_i q_j = 0) next to pairs with q_i q_j < 0."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_zero_slot_goldens', os.path.join(ROOT, 'scripts', 'record_zero_slot_goldens.py'))
Z = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(Z)


def _oo_distances(c):
    o, L = c['positions'][0::3], c['box']
    d = o[:, None, :] - o[None, :, :]
    d -= L * np.round(d / L)
    return np.sqrt((d * d).sum(-1))


@pytest.mark.parametrize('name', sorted(Z.CASES))
def test_zero_slot_bit_identical(name):
    case = Z.CASES[name]
    c, out, info = Z.run_case(case)
    two = dict(case['options']).get('fuse_rows', 1) == 0
    assert info['near']['list_kind'] == 1 and info['near']['has_site_table'] == 1 and info['outer']['has_site_table'] == 1
    assert info['near']['rode_along'] == (0 if two else 1)          # fused step-boundary pass, or two launches of their own
    lane_trips, entries = info['padding']
    print('%s: %d lane-trips for %d row entries' % (name, lane_trips, entries))
    assert lane_trips > entries > 0          # padding lanes: rows are no multiple of their lanes, and a wavefront walks to its longest row

    # the path the case is about was taken
    if case['change'] == 'edges':
        x = c['positions']
        for anchor, j, want in Z.edge_pairs(Z.T.make_system(dict(case, change=None))):
            d = x[3 * j] - x[3 * anchor]
            assert d[1] == 0.0 and Z.r2_of(float(d[0]), float(d[2])) == want
        wants = sorted(w for _, _, w in Z.edge_pairs(Z.T.make_system(dict(case, change=None))))
        assert wants == [np.nextafter(0.7 * 0.7, 0.0), 0.7 * 0.7, np.nextafter(1.0, 0.0), 1.0]
    if case['change'] == 'push':
        d_oh, d_oo = Z.T.closest_pairs(c)
        assert d_oh < Z.T.TABLE_END and d_oo < 0.7 * Z.T.SIGMA_O
    if case['change'] == 'q0':
        assert np.sum(c['charge'] == 0.0) > 100
    if case['change'] is None:
        # listed partners beyond the tables' last interval: a table ends one interval (less than 0.4 % in r) above its cutoff
        d = _oo_distances(c)
        for rc in (Z.RC_NEAR, Z.RC_OUTER):
            assert np.sum((d > 1.02 * rc) & (d < rc + Z.SKIN)) > 100
    if case['change'] == 'lattice':
        d = _oo_distances(c)
        np.fill_diagonal(d, np.inf)
        far = Z.lattice_far_molecules(case)
        # their nearest neighbours are listed (first atoms within list radius + twice the extent) and out of reach of every atom pair
        assert np.all(np.abs(d[far].min(1) - Z.LATTICE_A) < 1e-9) and Z.LATTICE_A - 4 * 0.0958 / 2 > Z.RC_OUTER
        assert info['outer']['n_list_pairs'] > 0
        atoms = (3 * far[:, None] + np.arange(3)).ravel()
        for key in ('f1', 'f2'):
            assert np.all(out[key][atoms] == 0.0) and not np.any(np.signbit(out[key][atoms])), key
        assert np.abs(out['f2']).max() > 1.0          # (the pairs moved to 0.9 nm feel the outer force)

    gold = dict(np.load(Z.golden_path(name)))
    keep = Z.P.golden_atoms(len(c['positions']))
    for key in Z.KEYS:
        got = out[key][keep]
        print('%s %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, key, np.abs(got - gold[key]).max(), np.abs(gold[key]).max()))
    for key in Z.KEYS:
        got = out[key][keep]
        assert np.array_equal(got, gold[key]), key
        assert np.array_equal(np.signbit(got), np.signbit(gold[key])), key
        assert Z.digest(out[key]) == str(gold['sha_' + key]), key
    if case.get('same_f1'):
        # the guest of the fused pass and the stand-alone near launch: the same bits, every atom
        other = np.load(Z.golden_path(case['same_f1']))
        assert Z.digest(out['f1']) == str(other['sha_f1'])
