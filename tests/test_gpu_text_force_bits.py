"""GPU test of the force families that evaluate a user-written energy text (csrc/pair_expr.hip, term_expr.hip, cv.hip, compound.hip,
hbond.hip, manyparticle.hip) and of the CMAP force, which shares their gather and block reduction: energies and forces are the BITS
of the goldens under tests/golden/text_force_*.npz.

The goldens were recorded by scripts/record_text_force_goldens.py with the build of the commit before csrc/expr_force.h stated the
families' shared pieces once; that file has the cases (the smallest shapes at which each shared piece can go wrong) and the three
evaluations each of them runs: with the energy, without it, and accumulating onto a buffer that holds numbers.  Bit equality is
what fits: these kernels use no atomics and keep fp contraction off.  No pair, term or set of a case is left out of the comparison."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_text_force_goldens', os.path.join(ROOT, 'scripts', 'record_text_force_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@pytest.mark.parametrize('name', list(R.CASES))
def test_same_bits_as_before_the_shared_header(name):
    golden = np.load(R.golden_path(name))
    positions, energy, forces = R.run_case(name)
    assert np.array_equal(positions, golden['positions']), 'the case is not the one that was recorded'
    worst = np.abs(forces - golden['forces']).max()
    print('%s: E = %s (golden %s), max|dF| = %.3e' % (name, energy, golden['energy'], worst))
    assert golden['energy'].dtype == np.float64 and golden['forces'].dtype == np.float64
    assert np.array_equal(energy, golden['energy'])
    assert np.array_equal(forces, golden['forces'])
