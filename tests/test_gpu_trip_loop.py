"""The trip loop of the molecule-row pair kernels (csrc/cluster.hip: k_cpair / cwalk_rows) reads its arguments in place, where they
are used, keeps the table look-up's per-lane choices in vector registers, combines a pair's lane conditions before the one select
and leaves out the guest's sum with an exact zero.  None of it may change a bit of what the kernels compute: forces of one evaluation
and the state after 6 outer steps of RESPA [4, 2, 1] equal the goldens recorded by the build of the commit before
(scripts/record_trip_loop_goldens.py, kernel revision r06-prologue), and the forces meet the CPU oracle at the tolerance of
tests/test_gpu_abi_parity.py (1e-9 of the largest force).

Cases = what tests/test_gpu_pair_prologue.py does not reach (scripts/record_trip_loop_goldens.py: CASES): pairs below the tables
(the analytic branch of host and guest), chargeless hydrogens (signed zeros), two classes of sites (the kernels without site-site
tables, whose guest keeps its Lennard-Jones sum), NonbondedForce hosts (Ewald direct space, reaction field; also as one fused
launch of the two pair forces alone: no epilogue), the inner loop as launches of its own, a box with interior tasks."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_trip_loop_goldens', os.path.join(ROOT, 'scripts', 'record_trip_loop_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _pair_eval(d, c):
    return O.pair_eval(d, c['positions'], c['box'], c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'], use_cells=len(c['positions']) > 1536)[1]


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_trip_loop_bit_identical_and_vs_oracle(name):
    case = R.CASES[name]
    c, out, info = R.run_case(case)
    assert info['near']['list_kind'] == 1 and info['near']['rode_along'] == 1          # molecule rows, fused step-boundary pass
    # the path the case is about was taken
    if name == 'pushed_water':
        d_oh, d_oo = R.closest_pairs(c)
        print('%s: closest O-H %.4f nm (table end %.3f), closest O-O %.4f nm (0.7 sigma = %.4f)' % (name, d_oh, R.TABLE_END, d_oo, 0.7 * R.SIGMA_O))
        assert d_oh < R.TABLE_END and d_oo < 0.7 * R.SIGMA_O
    if name == 'neutral_hydrogens':
        assert np.sum(c['charge'] == 0.0) > 100 and info['near']['has_site_table'] == 1
    if name == 'two_site_classes':
        assert info['near']['has_site_table'] == 0 and info['outer']['has_site_table'] == 0
    else:
        assert info['near']['has_site_table'] == 1 and info['outer']['has_site_table'] == 1
    if name == 'launches_of_their_own':
        assert info['run']['epilogues'] == 0
    if name in ('pushed_water', 'neutral_hydrogens', 'box17_interior'):
        assert info['run']['epilogues'] > 0
    if case.get('direct'):
        assert info['direct_near']['rode_along'] == 1 and info['direct_outer']['list_kind'] == 1 and info['direct_outer']['has_site_table'] == 1
    if name == 'box17_interior':
        # rows whose molecules are farther from every face than the list's reach take the walk without a periodic image: the box
        # (5.28 nm) is more than four times the outer cutoff plus buffer
        assert c['box'].min() > 4.0 * 1.1

    gold = dict(np.load(R.golden_path(name)))
    if case.get('direct'):
        gold.update(np.load(R.golden_path(name + '_direct')))
    keep = R.P.golden_atoms(len(c['positions']))
    keys = ['f1', 'f2', 'x', 'v'] + (['fd1', 'fd2'] if case.get('direct') else [])
    got = {key: out[key][keep] for key in keys}
    for key in keys:
        print('%s %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, key, np.abs(got[key] - gold[key]).max(), np.abs(gold[key]).max()))

    # the oracle: group 1 is the near force; group 2 is one pair force where the outer force is the DampedSmoothedForce (its
    # discount of the near force is group 31).  A NonbondedForce in group 2 brings more than its pair part (reciprocal space,
    # exceptions, the discount): there the two pair forces of the fused launch alone meet the oracle.
    checks = [('f1', O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5))]
    if case['outer'] == 'damped':
        checks.append(('f2', O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1)))
    if case.get('direct'):
        dn, dh = R.direct_descs(case)
        checks += [('fd1', dn), ('fd2', dh)]
    errs = {}
    for key, d in checks:
        f_ref = _pair_eval(d, c)
        errs[key] = (np.abs(out[key] - f_ref).max(), np.abs(f_ref).max())          # (every atom, whatever the golden keeps)
        print('%s %s: max |new - oracle| / max |oracle| = %.3e' % (name, key, errs[key][0] / errs[key][1]))

    for key in keys:
        assert np.array_equal(got[key], gold[key]), key
    for key, (err, scale) in errs.items():
        assert err <= 1e-9 * scale, key
