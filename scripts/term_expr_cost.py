"""What the generic term-expression kernels cost: one force-only evaluation of 100 000 synthetic torsions written as the text
`k*(1+cos(n*theta-theta0))` -- compiled by expr.compile_term and interpreted per term by csrc/term_expr.hip -- against the same
terms as AMM_TORSION_PERIODIC on the hand-written term-parallel path of csrc/bonded.hip, and the same pair of measurements for
100 000 harmonic bonds (`0.5*k*(r-r0)^2` against AMM_BOND_HARMONIC).  Every path is two launches (terms, then the per-atom gather);
the time is that of both, from HIP events on the launch stream around --reps evaluations after a warm-up.

    python scripts/term_expr_cost.py [--reps 50] [--out profiles/term_expr_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TERMS = 100000
TEXTS = dict(torsion=('k*(1+cos(n*theta-theta0))', ('theta',), ['n', 'theta0', 'k']), bond=('0.5*k*(r-r0)^2', ('r',), ['r0', 'k']))


def helix(n):
    """n atoms on a helix (0.15 nm between neighbours, no three of them collinear) with a little noise: a chain without a box."""
    t = np.arange(n)
    x = np.stack([0.1 * np.cos(1.1 * t), 0.1 * np.sin(1.1 * t), 0.11 * t], axis=1)
    return x + np.random.default_rng(2024).normal(scale=0.005, size=x.shape)


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'term_expr_cost.txt'))
    args = ap.parse_args()
    n = TERMS + 3
    rng = np.random.default_rng(7)
    ctx = B.HipContext(n, None)
    x = torch.as_tensor(helix(n), dtype=torch.float64, device='cuda')
    t = np.arange(TERMS)
    rows = dict(torsion=np.stack([t, t + 1, t + 2, t + 3], axis=1), bond=np.stack([t, t + 1], axis=1))
    params = dict(torsion=np.stack([rng.integers(1, 4, TERMS).astype(float), rng.uniform(0.0, 3.0, TERMS), rng.uniform(1.0, 10.0, TERMS)], axis=1),
                  bond=np.stack([rng.uniform(0.14, 0.16, TERMS), rng.uniform(1e5, 3e5, TERMS)], axis=1))
    kinds = dict(torsion=(B.TERM_TORSION, B.TORSION_PERIODIC), bond=(B.TERM_BOND, B.BOND_HARMONIC))
    lines = ['term-expression kernels against the hand-written term-parallel path, %d synthetic terms on a helix of %d atoms, force only' % (TERMS, n),
             'kernel revision %s, %d evaluations each (two launches: terms, gather), HIP events on the stream' % (B.kernel_revision(), args.reps)]
    for what in ('torsion', 'bond'):
        text, variables, names = TEXTS[what]
        prog = X.compile_term(text, variables, names, [])
        idx = np.full((TERMS, 4), -1, dtype=np.int32)
        idx[:, :rows[what].shape[1]] = rows[what]
        generic = ctx.term_expr_create(kinds[what][0], prog.code, prog.consts, [], idx, params[what].T)
        hand = ctx.bonded_create()
        ctx.bonded_add_terms(hand, kinds[what][1], rows[what], params[what])
        ctx.bonded_finalize(hand)
        us, forces = {}, {}
        for label, fid in (('hand-written', hand), ('generic', generic)):
            f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
            for _ in range(3):
                ctx.force_eval(fid, x, f)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.reps):
                ctx.force_eval(fid, x, f)
            stop.record()
            ctx.synchronize()
            us[label] = 1e3 * start.elapsed_time(stop) / args.reps
            forces[label] = f.cpu().numpy()
        ctx.check()
        a, b = forces['hand-written'], forces['generic']
        lines += ['%s text: %s (%d code words)' % (what, text, len(prog.code)),
                  '  hand-written (bonded.hip, kind %d): %8.1f us' % (kinds[what][1], us['hand-written']),
                  '  generic      (term_expr.hip)      : %8.1f us' % us['generic'],
                  '  ratio generic / hand-written: %.2f   max |F_generic - F_hand| = %.3e of max |F| = %.6g' %
                  (us['generic'] / us['hand-written'], np.abs(a - b).max(), np.abs(a).max())]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
