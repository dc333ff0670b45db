"""What the generic pair-expression kernel costs: force-only evaluation of the near Lennard-Jones potential of config C2 (32 768 atoms,
atomsmm_amd.testing.lj_fluid) written as a text the HIP path does NOT recognise -- compiled by expr.compile_pair and interpreted per
pair by csrc/pair_expr.hip -- against the recognised NearNonbondedForce(rc, rs, None) on its hand-written kernel.  Both forces walk
per-atom neighbour rows built with the same Verlet buffer; the time is that of the pair kernel alone, from HIP events on the launch
stream (amm_profile_enable), averaged over --reps launches after a warm-up.

    python scripts/pair_expr_cost.py [--reps 50] [--out profiles/pair_expr_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXT = ('S*4*epsilon*((sigma/r)^12-(sigma/r)^6); S = 1 + step(r - rs0)*u^3*(15*u - 6*u^2 - 10); u = (r - rs0)/(rc0 - rs0); '
        'sigma = 0.5*(sigma1+sigma2); epsilon = sqrt(epsilon1*epsilon2)')


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    from atomsmm_amd.forces import describe_energy
    from atomsmm_amd.testing import lj_fluid
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--skin', type=float, default=0.2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pair_expr_cost.txt'))
    args = ap.parse_args()
    case = lj_fluid(32)
    n = len(case['positions'])
    sigma = float(case['sigma'][0])
    rc, rs = 2.5 * sigma, 0.9 * 2.5 * sigma
    assert describe_energy(TEXT, dict(rc0=rc, rs0=rs)) is None
    prog = X.compile_pair(TEXT, ['sigma', 'epsilon'], ['rc0', 'rs0'])
    ctx = B.HipContext(n, case['box'])
    x = torch.as_tensor(case['positions'], dtype=torch.float64, device='cuda')
    f = [torch.zeros((n, 3), dtype=torch.float64, device='cuda') for _ in range(2)]
    family = ctx.pair_create(B.pair_desc(B.NEAR_NONE, rc, rc0=rc, rs0=rs), case['charge'], case['sigma'], case['epsilon'], skin=args.skin)
    generic = ctx.pair_expr_create(B.pair_desc(B.PAIR_EXPR, rc), prog.code, prog.consts, [dict(rc0=rc, rs0=rs)[g] for g in prog.globals_],
                                   case['sigma'], case['epsilon'], None, skin=args.skin)
    us = {}
    for label, fid, buf in (('family', family, f[0]), ('generic', generic, f[1])):
        for _ in range(3):
            ctx.force_eval(fid, x, buf)
        ctx.profile_enable(True, only=fid)
        for _ in range(args.reps):
            ctx.force_eval(fid, x, buf)
        ctx.synchronize()
        count, ms = ctx.profile_read(fid)
        ctx.profile_enable(False)
        assert count == args.reps
        us[label] = 1e3 * ms / count
    ctx.check()
    a, b = f[0].cpu().numpy(), f[1].cpu().numpy()
    stats = {k: ctx.pair_stats(fid) for k, fid in (('family', family), ('generic', generic))}
    lines = [
        'pair-expression kernel against the hand-written near kernel, config C2 (%d atoms, rc = %.3f nm, Verlet buffer %.2f nm), force only' % (n, rc, args.skin),
        'kernel revision %s, %d launches each, HIP events around the pair kernel' % (B.kernel_revision(), args.reps),
        'text: %s' % TEXT,
        'program: %d code words, %d constants, %d globals' % (len(prog.code), len(prog.consts), len(prog.globals_)),
        'family  (NEAR_NONE, list_kind %d, table %d, chargeless %d): %9.1f us' % (stats['family']['list_kind'], stats['family']['has_table'],
                                                                                 stats['family']['chargeless'], us['family']),
        'generic (PAIR_EXPR, list_kind %d, %d lanes per atom)      : %9.1f us' % (stats['generic']['list_kind'], stats['generic']['lanes_per_atom'],
                                                                                  us['generic']),
        'ratio generic / family: %.1f' % (us['generic'] / us['family']),
        'list entries %d, max |F_generic - F_family| = %.3e of max |F| = %.6g' % (stats['generic']['n_list_pairs'], np.abs(a - b).max(), np.abs(a).max()),
    ]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
