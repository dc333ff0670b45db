"""The list build of the molecule rows (csrc/cluster.hip: k_cbuild) takes a cell's stencil tables -- piece starts, stream prefix,
periodic shift codes, coarse table -- from the record that the rebuild's sort launch (k_csort_gather: cbuild_tables) wrote for the
cell, instead of making them in each of the cell's wavefronts, and drains a row's leftover of at most 64 survivors one per lane.
Rows must stay what they were, entry for entry and in place: entries are dealt to a row's lanes by position, so equal force bits
prove equal rows.  Forces of the near and of the outer force and the list's entry counts equal the goldens recorded by the build of
the commit before (scripts/record_build_tables_goldens.py, kernel revision r07-triploop).

Cases (scripts/record_build_tables_goldens.py: CASES) = the smallest shapes that reach each path: 1 536 atoms (3 cells per edge: the
per-pair-image instantiation, a stencil that wraps onto itself), 14 739 atoms (7 cells per edge: shift codes, interior and edge
cells) and the same box after every molecule was moved beyond the Verlet buffer (a second build, whose tables must be its own), two
Verlet buffers on 5 184 atoms that leave every row a leftover of 1 survivor (one-per-lane drain) and of 123 (packed drain), and two
ranks' slices of the rows at 1 536 and 5 184 atoms (the slice instantiations)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_build_tables_goldens', os.path.join(ROOT, 'scripts', 'record_build_tables_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@functools.lru_cache(maxsize=None)
def _results(name):
    return R.run_case(R.CASES[name])


def _compare(name, tags):
    case = R.CASES[name]
    c, results = _results(name)
    gold = dict(np.load(R.golden_path(name)))
    assert len(results) == case['world']
    for r, out in enumerate(results):
        rows = R.P.golden_atoms(len(c['positions']))
        for tag in tags:
            for key in ('f1' + tag, 'f2' + tag):
                g = gold['r%d_%s' % (r, key)]
                print('%s rank %d %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, r, key, np.abs(out[key][rows] - g).max(), np.abs(g).max()))
            for key in ('pairs_near' + tag, 'pairs_outer' + tag):
                print('%s rank %d %s: %d (golden %d)' % (name, r, key, out[key], gold['r%d_%s' % (r, key)]))
    for r, out in enumerate(results):
        rows = R.P.golden_atoms(len(c['positions']))
        for tag in tags:
            for key in ('f1' + tag, 'f2' + tag):
                assert np.array_equal(out[key][rows], gold['r%d_%s' % (r, key)]), (r, key)
                assert R.digest(out[key]) == str(gold['r%d_%s_sha256' % (r, key)]), (r, key)          # every atom
            for key in ('pairs_near' + tag, 'pairs_outer' + tag):
                assert out[key] == gold['r%d_%s' % (r, key)] and out[key] > 0, (r, key)
    return c, results


@pytest.mark.parametrize('name', ['box8', 'box17'])
def test_first_build_rows_bit_identical(name):
    c, results = _compare(name, [''])
    print('%s: %d cells' % (name, results[0]['n_cells']))
    # (fewer than 5 cells per edge: images per atom pair and a stencil of the whole box; 5 or more: shift codes)
    assert (results[0]['n_cells'] < 125) == (name == 'box8')
    assert results[0]['builds'] >= 1


def test_second_build_uses_its_own_tables():
    c, results = _compare('box17', ['_moved'])
    out = results[0]
    moved = np.linalg.norm(R.displaced(c) - c['positions'], axis=1)
    print('box17 moved: largest displacement %.3f nm, builds %d -> %d' % (moved.max(), out['builds'], out['builds_moved']))
    assert moved.max() > 0.5 * (out['rlist'] - R.RC_OUTER)          # beyond what the buffer allows
    assert out['builds_moved'] == out['builds'] + 1                # a rebuild happened
    assert out['pairs_outer_moved'] != out['pairs_outer']          # with other rows


@pytest.mark.parametrize('name,lo,hi', [('box12_leftover_1', 1, 64), ('box12_leftover_123', 65, 127)])
def test_final_drain_of_each_width(name, lo, hi):
    c, results = _compare(name, [''])
    out = results[0]
    assert out['rlist'] == pytest.approx(R.RC_OUTER + R.CASES[name]['skin'], abs=1e-12)
    left = R.sphere_counts(c, R.CASES[name]['skin']) % 128
    print('%s: leftover survivors of a row, min %d max %d; builds %d' % (name, left.min(), left.max(), out['builds']))
    assert lo <= left.min() and left.max() <= hi
    assert out['builds'] >= 1


@pytest.mark.parametrize('name', ['box8_two_ranks', 'box12_two_ranks'])
def test_slices_of_two_ranks(name):
    c, results = _compare(name, [''])
    n = len(c['positions'])
    assert sum(int(out['slice_atoms']) for out in results) == n and all(0 < out['slice_atoms'] < n for out in results)
    for out in results:
        assert out['builds'] >= 1
        assert np.array_equal(out['f1'], results[0]['f1']) and np.array_equal(out['f2'], results[0]['f2'])
