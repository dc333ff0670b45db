"""The zero-slot instantiations of the molecule-row pair kernels (csrc/cluster.hip: k_cpair / cwalk_rows) no longer subtract the
zone's base interval from a pair's raw interval: the zone select delivers `table address - 48 x base of the zone` and the look-up
forms raw x 48 + that (csrc/pair_tab.h: amm_tab_fetch_pass); the guest of a fused pass whose factor relative to the host is exactly
1.0 leaves the product by it out.  Neither may change a bit, or the sign of a zero, of any force: forces of one evaluation and the
state after 6 outer steps of RESPA [4, 2, 1] equal the goldens recorded by the build of the commit before
(scripts/record_lookup_offset_goldens.py, kernel revision r09-zeroslot) -- array_equal and equal sign bits on the atoms a golden
keeps, the SHA-256 of the bytes of ALL atoms.

Cases (scripts/record_lookup_offset_goldens.py: CASES), at the smallest boxes that reach each loop: 1 536 atoms (3 cells per edge:
the per-pair-image loop) and 14 739 atoms (7 cells: interior and image/molecule tasks), each as the fused step-boundary pass and as
two launches of their own -- the near force has the same bits either way:
  * a plain liquid;
  * table_ends: a pair in the first interval of zone A and one in the last interval of zone B a counting pair reads, of the Coulomb
    table (oxygen - hydrogen) and of the site-site table (two oxygens), of the near and of the outer force: the two ends of each
    offset.  (In the fused pass a pair below the LARGER of the two forces' lower ends is redone analytically for both, so the near
    table's own first interval is read by the two-launch form only; the fused form reads the outer table's.)
  * zone_boundary: pairs with w = r^2 x scale = 1 and the double below it, Coulomb and site-site, near and outer table;
  * cutoff_edges: r^2 = rc^2 and the last double below it at both cutoffs;
  * pushed_water: a pair below the tables inside trips of ordinary pairs -- the analytic redo and the guest's `!lowp`.  Its entry is a
    front entry.  A back entry cannot hold such a pair: the list build files a molecule pair in the front part of a row when the
    smallest of its nine atom-pair distances is below the near list radius, and a rebuild comes long before an atom has moved
    the 0.6 nm that would take a back entry's pair below a table; no system that can be built through the API has one.
  * neutral_hydrogens: chargeless hydrogens (q_i q_j = 0) next to pairs with q_i q_j < 0;
  * lattice_outside: molecules all of whose listed partners are outside the cutoffs (force +0.0, sign bit clear);
  * discount: a fused evaluation whose gfac is not 1.0 -- FarNonbondedForce, whose discount (sign -1) rides on the total's walk:
    it must take the instantiation that multiplies by gfac and match its golden."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_lookup_offset_goldens', os.path.join(ROOT, 'scripts', 'record_lookup_offset_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
Z = R.Z


def _check_placements(c, case):
    """The placed pairs are where the case wants them: r^2 exact, and the interval each reads is the end / side it is named for."""
    near, outer = R.fines()
    assert near['bad'] == 0 and outer['bad'] == 0
    lay = R.layouts(near['fine'], outer['fine'])
    for which, res in (('near', near), ('outer', outer)):          # the layout this file works out is the library's
        assert lay[which]['nint'] == res['nint'] and lay[which]['ss_first'] == res['ss_first'] and lay[which]['nA'] == res['n_below_kink']
    x = c['positions']
    assert len(c['placed']) == 8
    for name, i, j, want, which, site in c['placed']:
        d = x[j] - x[i]
        assert d[1] == 0.0 and Z.r2_of(float(d[0]), float(d[2])) == want, name
        L = lay[which]
        w, idx = R.interval_of(L, want)
        print('%s: r = %.6f nm, w = %.17g, interval %d of %d (site-site from %d)' % (name, np.sqrt(want), w, idx, L['nint'], L['ss_first']))
        if name.endswith('coulomb_first'):
            assert idx == 0 and want >= L['r2min']
        elif name.endswith('site_first'):
            assert idx == L['ss_first'] and want >= L['ss_r2min']
        elif name.endswith('_last'):
            assert idx == {'near': near, 'outer': outer}[which]['idx_max'] and idx <= L['nint'] - 2 and w >= 1.0
        elif name.endswith('w1_at'):
            assert w == 1.0 and idx == L['nA']
        elif name.endswith('w1_below'):
            assert w == np.nextafter(1.0, 0.0) and idx == L['nA'] - 1
        else:
            raise AssertionError(name)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_lookup_offset_bit_identical(name):
    case = R.CASES[name]
    c, out, info = R.run_case(case)
    two = dict(case['options']).get('fuse_rows', 1) == 0
    assert info['near']['list_kind'] == 1 and info['near']['has_site_table'] == 1 and info['outer']['has_site_table'] == 1
    assert info['near']['rode_along'] == (0 if two else 1)          # fused step-boundary pass, or two launches of their own
    if not two:
        # what RESPASystem builds: both forces with the same Coulomb constant and sign -- the kernel without the product
        assert info['guest_factor'] == (1.0, True)
    lane_trips, entries = info['padding']
    assert lane_trips > entries > 0

    # the path the case is about was taken
    if case['change'] in ('ends', 'boundary'):
        _check_placements(c, case)
    if case['change'] == 'edges':
        x = c['positions']
        pairs = Z.edge_pairs(Z.T.make_system(dict(case, change=None)))
        for anchor, j, want in pairs:
            d = x[3 * j] - x[3 * anchor]
            assert d[1] == 0.0 and Z.r2_of(float(d[0]), float(d[2])) == want
        assert sorted(w for _, _, w in pairs) == [np.nextafter(0.7 * 0.7, 0.0), 0.7 * 0.7, np.nextafter(1.0, 0.0), 1.0]
    if case['change'] == 'push':
        d_oh, d_oo = Z.T.closest_pairs(c)
        assert d_oh < Z.T.TABLE_END and d_oo < 0.7 * Z.T.SIGMA_O
    if case['change'] == 'q0':
        assert np.sum(c['charge'] == 0.0) > 100
    if case['change'] == 'lattice':
        far = Z.lattice_far_molecules(case)
        assert info['outer']['n_list_pairs'] > 0
        atoms = (3 * far[:, None] + np.arange(3)).ravel()
        for key in ('f1', 'f2'):
            assert np.all(out[key][atoms] == 0.0) and not np.any(np.signbit(out[key][atoms])), key
        assert np.abs(out['f2']).max() > 1.0

    gold = dict(np.load(R.golden_path(name)))
    keep = Z.P.golden_atoms(len(c['positions']))
    for key in R.KEYS:
        got = out[key][keep]
        print('%s %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, key, np.abs(got - gold[key]).max(), np.abs(gold[key]).max()))
    for key in R.KEYS:
        got = out[key][keep]
        assert np.array_equal(got, gold[key]), key
        assert np.array_equal(np.signbit(got), np.signbit(gold[key])), key
        assert Z.digest(out[key]) == str(gold['sha_' + key]), key
    if case.get('same_f1'):
        # the guest of the fused pass and the stand-alone near launch: the same bits, every atom
        other = np.load(R.golden_path(case['same_f1']))
        assert Z.digest(out['f1']) == str(other['sha_f1'])


def test_guest_of_opposite_sign_takes_the_multiplying_kernel():
    """gfac = (Kc sign)_guest / (Kc sign)_host = -1: the fused pass of FarNonbondedForce (reaction-field total, discount of sign -1
    as its guest) runs the instantiation that multiplies by gfac, unchanged -- the same bits as the build of the commit before."""
    c, f2, info = R.run_discount()
    assert info['total']['list_kind'] == 1 and info['discount']['rode_along'] == 1 and info['discount']['has_site_table'] == 1
    assert info['guest_factor'] == (-1.0, False)
    gold = np.load(R.golden_path('discount'))
    print('discount f2: max |new - golden| = %.3e (max |golden| = %.3e)' % (np.abs(f2 - gold['f2']).max(), np.abs(gold['f2']).max()))
    assert np.array_equal(f2, gold['f2']) and np.array_equal(np.signbit(f2), np.signbit(gold['f2']))
    assert Z.digest(f2) == str(gold['sha_f2'])
