"""What a general CustomCVForce (csrc/cv.hip, AMM_FORCE_CV) costs next to the bonded group of the C3 box (98 304 atoms of flexible
TIP3P water: 65 536 harmonic bonds and 32 768 harmonic angles in one bond-list set).  The group's members are evaluated in order --
the first writes the buffer, the collective-variable force adds to it -- as the op scheduler's plain path does for a group that holds
such a force; force only; HIP events on the launch stream around --reps evaluations after a warm-up.

  * the group without the force: the bond-list set alone;
  * with 1, 2 and 8 collective variables that are one torsion each (H - O ... O - H of two neighbouring waters; the outer text sums
    harmonic restraints);
  * with one collective variable that is a bond-list set over every bond of the box (outer text 0.5*k*cv1^2).

A collective-variable force costs its K inner evaluations (each writes all 3n doubles of its block of the scratch) and the one launch
that runs the outer text and combines the K blocks: K + 1 reads and one write of 3n doubles.

    python scripts/cv_force_cost.py [--reps 50] [--nside 32] [--out profiles/cv_force_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    from atomsmm_amd.testing.synthetic import tip3p_box
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--nside', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cv_force_cost.txt'))
    args = ap.parse_args()
    c = tip3p_box(args.nside)
    n = len(c['positions'])
    ctx = B.HipContext(n, c['box'])
    x = torch.as_tensor(c['positions'], dtype=torch.float64, device='cuda')
    bond_par = np.stack([c['bond_r0'], c['bond_k']], axis=1)
    own = ctx.bonded_create()
    ctx.bonded_add_terms(own, B.BOND_HARMONIC, c['bonds'], bond_par, periodic=True)
    ctx.bonded_add_terms(own, B.ANGLE_HARMONIC, c['angles'], np.stack([c['angle_theta0'], c['angle_k']], axis=1), periodic=True)
    ctx.bonded_finalize(own)

    def torsion_cv(k):
        """theta of H1 - O of molecule 2k and O - H1 of its lattice neighbour 2k + 1 (the oxygens alone sit on a line)."""
        prog = X.compile_term('theta', ('theta',), [], [])
        idx = np.array([[6 * k + 1, 6 * k, 6 * k + 3, 6 * k + 4]], dtype=np.int32)
        return ctx.term_expr_create(B.TERM_TORSION, prog.code, prog.consts, [], idx, np.zeros((0, 1)), periodic=True)

    def torsion_case(n_cv):
        names = ['phi%d' % k for k in range(n_cv)]
        text = '+'.join('0.5*k*(%s-0.3)^2' % name for name in names)
        prog = X.compile_cv(text, names, [], ['k'])
        return ctx.cv_create([torsion_cv(k) for k in range(n_cv)], 0, prog.code, prog.consts, [100.0]), len(prog.code)

    def bond_case():
        inner = ctx.bonded_create()
        ctx.bonded_add_terms(inner, B.BOND_HARMONIC, c['bonds'], bond_par, periodic=True)
        ctx.bonded_finalize(inner)
        prog = X.compile_cv('0.5*k*cv1^2', ['cv1'], [], ['k'])
        return ctx.cv_create([inner], 0, prog.code, prog.consts, [1e-4]), len(prog.code)

    def time_group(members):
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')

        def evaluate():
            for k, fid in enumerate(members):
                ctx.force_eval(fid, x, f, accumulate=k > 0)
        for _ in range(3):
            evaluate()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            evaluate()
        stop.record()
        ctx.synchronize()
        ctx.check()
        return 1e3 * start.elapsed_time(stop) / args.reps

    lines = ['a CustomCVForce (csrc/cv.hip) in the bonded group of the C3 box: %d atoms, %d bonds + %d angles in one bond-list set, force only' % (
                 n, len(c['bonds']), len(c['angles'])),
             'kernel revision %s, %d evaluations each, members in order (the plain path), HIP events on the stream' % (B.kernel_revision(), args.reps)]
    base = time_group([own])
    lines.append('  the group without the force                         : %8.1f us' % base)
    for n_cv in (1, 2, 8):
        fid, words = torsion_case(n_cv)
        us = time_group([own, fid])
        lines.append('  + %d torsion CV%s of one term each (%3d code words)     : %8.1f us  (+%.1f us, %.1f us per CV and launch of the combine)' % (
            n_cv, ' ' if n_cv == 1 else 's', words, us, us - base, (us - base) / n_cv))
    fid, words = bond_case()
    us = time_group([own, fid])
    lines.append('  + one CV = harmonic bonds over every bond (%2d words)  : %8.1f us  (+%.1f us)' % (words, us, us - base))
    lines.append('scratch of the last force: %.1f MB (24 K n bytes)' % (24.0 * n / 1e6))
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
