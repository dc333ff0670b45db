"""The list build of the molecule rows (csrc/cluster.hip: k_cbuild) keeps a row's sphere constants, its ring's entry count and head in
scalar registers over the candidate stream, tests the rows of a batch in unrolled code (rows beyond the batch are skipped by a scalar
branch) and drains the rows whose ring holds 128 from a scalar pending mask; the drain forms its lane masks on the scalar side and
stores through a 32-bit offset from a scalar row base.  Rows must stay what they were, entry for entry and in place: entries are dealt
to a row's lanes by position, so equal force bits prove equal rows.  Forces of the near and of the outer force and the list's entry
counts equal the goldens recorded by the build of the commit before (scripts/record_build_loops_goldens.py, kernel revision
r10-lookupoffset).

Cases (scripts/record_build_loops_goldens.py: CASES) = the smallest shapes that reach each path; which paths a case reaches is worked
out on the CPU (stream_events) and asserted here:
  1 536 atoms (3 cells per edge: the per-pair-image instantiations, a stencil that wraps), 5 184 and 14 739 atoms;
  batches of 1, 2, 3, 4 and 5 rows (5 184 atoms: cells of 8, 12, 18 and 27 molecules in 5 parts);
  a stream of ONE chunk pair (375 atoms at a quarter of water's density), of 3 (1 029 atoms), of 4 and of 14 to 18 chunk pairs;
  5 184 atoms off the lattice at Verlet buffers of 0.05 and 0.12 nm: final drains of 1, 64 (one survivor per lane), 65 and 127 (two);
  up to five rows of a batch whose rings fill in the same chunk pair (the pending mask);
  rows that outgrow their capacity in a second build: the overflow is reported as before, the counts are what they were;
  the counting launch of every first build; two ranks' slices at 1 536 and 5 184 atoms (the slice instantiations);
  a second build after every molecule has moved beyond the buffer."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_build_loops_goldens', os.path.join(ROOT, 'scripts', 'record_build_loops_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@functools.lru_cache(maxsize=None)
def _results(name):
    return R.run_case(R.CASES[name])


@functools.lru_cache(maxsize=None)
def _events(name, second=False):
    return R.case_events(R.CASES[name], second)


def _compare(name, tags):
    case = R.CASES[name]
    c, results = _results(name)
    gold = dict(np.load(R.golden_path(name)))
    assert len(results) == case['world']
    rows = R.P.golden_atoms(len(c['positions']))
    checks = []
    for r, out in enumerate(results):
        for tag in tags:
            for key in ('f1' + tag, 'f2' + tag):
                if 'r%d_%s' % (r, key) not in gold and key not in out:
                    continue          # (an evaluation that ended in an error, then as now: its message is compared below)
                g = gold['r%d_%s' % (r, key)]
                print('%s rank %d %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, r, key, np.abs(out[key][rows] - g).max(), np.abs(g).max()))
                checks.append((r, key, True))
            for key in ('pairs_near' + tag, 'pairs_outer' + tag):
                print('%s rank %d %s: %d (golden %d)' % (name, r, key, out[key], gold['r%d_%s' % (r, key)]))
                checks.append((r, key, False))
    for r, key, is_force in checks:
        out, g = results[r], gold['r%d_%s' % (r, key)]
        if is_force:
            assert np.array_equal(out[key][rows], g), (r, key)
            assert R.digest(out[key]) == str(gold['r%d_%s_sha256' % (r, key)]), (r, key)          # every atom
        else:
            assert out[key] == g and out[key] > 0, (r, key)
    return c, results


def _model_matches(name, out, second=False):
    ev = _events(name, second)
    print('%s: %s' % (name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in ev.items()}))
    assert ev['n_cells'] == out['n_cells'], 'the CPU model of the build has other cells than the library'
    return ev


@pytest.mark.parametrize('name', ['box8', 'box12', 'box17'])
def test_first_build_rows_bit_identical(name):
    c, results = _compare(name, [''])
    out = results[0]
    ev = _model_matches(name, out)
    # (fewer than 5 cells per edge: images per atom pair and a stencil of the whole box; 5 or more: shift codes)
    assert (out['n_cells'] < 125) == (name == 'box8')
    assert out['builds'] >= 1          # (counting launch + build)
    assert ev['max_pending'] >= 4      # several rows of one batch fill their ring in the same chunk pair
    if name == 'box12':
        assert ev['batch_sizes'] == {1, 2, 3, 4, 5}
    if name == 'box17':
        assert any(n % 2 for n in ev['chunk_pairs']) and any(n % 2 == 0 for n in ev['chunk_pairs'])


@pytest.mark.parametrize('name,pairs', [('box5_sparse', 1), ('box7_sparse', 3)])
def test_short_streams(name, pairs):
    c, results = _compare(name, [''])
    ev = _model_matches(name, results[0])
    assert ev['chunk_pairs'] == {pairs}
    if pairs == 1:
        assert ev['full_drains'] == 0 and 64 < min(ev['leftovers'])         # everything is left to the final packed drain
    else:
        assert ev['max_pending'] == 5 and 0 < max(ev['leftovers']) <= 64     # five rows at once; then one survivor per lane


def test_second_build_after_every_molecule_moved():
    c, results = _compare('box17', ['_moved'])
    out = results[0]
    _model_matches('box17', out, second=True)
    moved = np.linalg.norm(R.displaced(c) - c['positions'], axis=1)
    print('box17 moved: largest displacement %.3f nm, builds %d -> %d' % (moved.max(), out['builds'], out['builds_moved']))
    assert moved.max() > 0.5 * (out['rlist'] - R.RC_OUTER)          # beyond what the buffer allows
    assert out['error_moved'] == ''
    assert out['builds_moved'] == out['builds'] + 1                # a rebuild happened
    assert out['pairs_outer_moved'] != out['pairs_outer']          # with other rows


@pytest.mark.parametrize('name,want', [('box12_shaken_s05', (1, 127)), ('box12_shaken_s12', (64, 65))])
def test_final_drains_of_both_forms(name, want):
    c, results = _compare(name, [''])
    out = results[0]
    assert out['rlist'] == pytest.approx(R.RC_OUTER + R.CASES[name]['skin'], abs=1e-12)
    ev = _model_matches(name, out)
    assert all(n in ev['leftovers'] for n in want)
    assert min(ev['leftovers']) <= 64 < max(ev['leftovers'])        # one survivor per lane AND two
    assert ev['batch_sizes'] == {1, 2, 3, 4, 5}


def test_rows_that_outgrow_their_capacity():
    c, results = _compare('box12_squeezed', ['', '_squeezed'])
    out = results[0]
    gold = dict(np.load(R.golden_path('box12_squeezed')))
    print('box12_squeezed: %r' % out['error_squeezed'])
    assert 'overflow' in out['error_squeezed']
    assert out['error_squeezed'] == str(gold['r0_error_squeezed'])          # the same longest row, the same capacity
    assert ('f1_squeezed' in out) == ('r0_f1_squeezed' in gold)
    assert out['builds_squeezed'] == out['builds'] + 1


@pytest.mark.parametrize('name', ['box8_two_ranks', 'box12_two_ranks'])
def test_slices_of_two_ranks(name):
    c, results = _compare(name, [''])
    n = len(c['positions'])
    assert sum(int(out['slice_atoms']) for out in results) == n and all(0 < out['slice_atoms'] < n for out in results)
    for out in results:
        assert out['builds'] >= 1
        assert np.array_equal(out['f1'], results[0]['f1']) and np.array_equal(out['f2'], results[0]['f2'])
