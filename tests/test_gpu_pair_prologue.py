"""The molecule-row pair kernels (csrc/cluster.hip: k_cpair) stage their tables from one image in global memory with every load in
flight at once, and fetch a task's row records ahead of the staging (first task) or behind the previous task's walk.  Neither may
change a bit of what they compute: forces of one evaluation and the state after 6 outer steps of RESPA [4, 2, 1] equal the goldens
recorded by the build of the commit before (scripts/record_pair_prologue_goldens.py, kernel revision r05-epi5), and the forces
meet the CPU oracle at the tolerance of tests/test_gpu_abi_parity.py (1e-9 of the largest force).

Cases = the smallest shapes where the new code can go wrong (scripts/record_pair_prologue_goldens.py: CASES).  The goldens of the
boxes above 1 536 atoms keep a seeded choice of 512 atoms (golden_atoms); the oracle comparison is over every atom."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('record_pair_prologue_goldens', os.path.join(ROOT, 'scripts', 'record_pair_prologue_goldens.py'))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def _oracle_forces(c, rc, rs, charge):
    """Group 1 of RESPASystem(rc, rs): the near force with force switch; group 2: DampedSmoothedForce(2.9, 1.0, 0.9) (the discount of
    the near force inside rc is group 31 and enters through the trajectory only)."""
    args = (c['positions'], c['box'], charge, c['sigma'], c['epsilon'], c['exc_pairs'])
    f1 = O.pair_eval(O.desc(O.NEAR_FSWITCH, rc=rc, rc0=rc, rs0=rs), *args)[1]
    f2 = O.pair_eval(O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1), *args)[1]
    return f1, f2


PHASE_COST = [0, 0, 1.0, 0.55, 0.32, 0.18, 0.11]          # csrc/cluster.hip: AMM_PHASE_COST


def _plan(nrows, shift, ncu):
    """The phases of a launch over `nrows` rows at 64 >> shift rows per task, as csrc/cluster.hip plans them (launch_cpair_t: one
    block of 8 wavefronts per CU, at most one block per 8 tasks, whole multiples of 8 blocks; cpair_plan_rec with row_phases on):
    [(shift, tasks per XCD), ...]."""
    ntask = -(-nrows // (64 >> shift))
    nblk = max(8, -(-min(ncu, -(-ntask // 8)) // 8) * 8)
    waves = (nblk >> 3) * 8
    plan = []

    def rec(rows, s, put):
        rpw = 64 >> s
        per_round = waves * rpw
        full, left = rows // per_round, rows % per_round
        finish = -(-rows // per_round) * PHASE_COST[s]
        s2, split = 6, 1e300
        for t in range(s + 1, 7):
            if left > 0:
                v = rec(left, t, False)
                if v < split:
                    split, s2 = v, t
        split += full * PHASE_COST[s]
        if left == 0 or s == 6 or finish <= split:
            if put:
                plan.append((s, -(-rows // rpw)))
            return finish
        if put and full > 0:
            plan.append((s, full * waves))
        rec(left, s2, put)
        return split

    rec(-(-nrows // 8), shift, True)
    return plan


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_pair_prologue_bit_identical_and_vs_oracle(name):
    case = R.CASES[name]
    c, out = R.run_case(case)
    assert out['list_kind'] == 1                    # molecule rows: the kernels this test is about
    if name == 'box14_two_tasks':
        # 64 lanes per row = one row per task: 2 744 tasks, 343 per XCD, on (CUs / 8) x 8 wavefronts per XCD (one block of 512 per
        # CU, launch_cpair_t) -- more than one task per wavefront on any chip with fewer than 343 CUs (the library does not report
        # its task count; this is the launch arithmetic of launch_cpair_t / cpair_plan)
        import torch
        assert len(c['positions']) // 3 // 8 > torch.cuda.get_device_properties(0).multi_processor_count
    if name == 'box17_two_phases':
        # a plan of two phases in which a wavefront has a task in each, so that its walk of tasks crosses the phase boundary: the
        # library does not report its plan; _plan below is the arithmetic of launch_cpair_t / cpair_plan for this device
        import torch
        plan = _plan(len(c['positions']) // 3, 5, torch.cuda.get_device_properties(0).multi_processor_count)
        print('%s: plan (lanes-per-row shift, tasks per XCD) = %s' % (name, plan))
        assert len(plan) >= 2 and all(ntask >= 1 for _, ntask in plan)          # wavefront 0 of every XCD takes task 0 of each phase
    gold = np.load(R.golden_path(name))
    keep = R.golden_atoms(len(c['positions']))
    keys = ['f1', 'f2', 'x', 'v'] + (['f1_rescaled', 'f2_rescaled'] if case.get('rescale') else [])
    full = {key: out[key] for key in ('f1', 'f2')}
    out = {key: out[key][keep] for key in keys}
    for key in keys:
        diff = np.abs(out[key] - gold[key]).max()
        print('%s %s: max |new - golden| = %.3e (max |golden| = %.3e)' % (name, key, diff, np.abs(gold[key]).max()))
    ref = _oracle_forces(c, case['rc'], case['rs'], c['charge'])
    for key, f_ref in zip(('f1', 'f2'), ref):
        print('%s %s: max |new - oracle| / max |oracle| = %.3e' % (name, key, np.abs(full[key] - f_ref).max() / np.abs(f_ref).max()))
    for key in keys:
        assert np.array_equal(out[key], gold[key]), key
    for key, f_ref in zip(('f1', 'f2'), ref):          # (every atom, whatever the golden keeps)
        assert np.abs(full[key] - f_ref).max() <= 1e-9 * np.abs(f_ref).max(), key
    if case.get('rescale'):
        # the second evaluation, at unchanged positions: the kernels must have staged the tables of the NEW charges
        ref = _oracle_forces(c, case['rc'], case['rs'], case['rescale'] * c['charge'])
        for key, f_ref in zip(('f1_rescaled', 'f2_rescaled'), ref):
            err = np.abs(out[key] - f_ref[keep]).max() / np.abs(f_ref).max()
            print('%s %s: max |new - oracle| / max |oracle| = %.3e' % (name, key, err))
            assert err <= 1e-9, key
