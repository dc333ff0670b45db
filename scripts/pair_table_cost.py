"""What a tabulated function costs in the generic pair-expression kernel (csrc/pair_expr.hip): force-only evaluations on config C2
(32 768 atoms, atomsmm_amd.testing.lj_fluid, the box and neighbour rows of scripts/pair_expr_cost.py) of

  * the Buckingham potential with mixing rules, A*exp(-B*r) - C/r^6 over three per-particle parameters, against the same potential
    with three Discrete2DFunction tables over a per-particle type, A(t1,t2)*exp(-B(t1,t2)*r) - C(t1,t2)/r^6 (two types);
  * a radial potential in closed form, 1e5*exp(-30*r) - 3e-3/r^6, against a Continuous1DFunction of 901 knots of it, U(r).

The time is that of the pair kernel alone, from HIP events on the launch stream (amm_profile_enable), averaged over --reps launches
after a warm-up; every variant is measured --rounds times, in turn, and the spread of the rounds is printed beside the mean.

    python scripts/pair_table_cost.py [--reps 50] [--rounds 3] [--out profiles/pair_expr_tables.txt] [--overwrite]

The lines are appended to --out (profiles/pair_expr_tables.txt also holds the comparison of programs without tables against the
parent commit, which this script does not make); --overwrite replaces the file.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXING = 'A*exp(-B*r)-C/r^6; A=sqrt(A1*A2); B=0.5*(B1+B2); C=sqrt(C1*C2)'
TABLES = 'A(t1,t2)*exp(-B(t1,t2)*r) - C(t1,t2)/r^6'
CLOSED = '1e5*exp(-30*r) - 3e-3/r^6'
SPLINE = 'U(r)'
PER_TYPE = np.array([[1.1e5, 36.0, 2.5e-3], [4.0e4, 30.0, 4.5e-3]])          # A, B, C of the two types


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    from atomsmm_amd import tables as T
    from atomsmm_amd.testing import lj_fluid
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--skin', type=float, default=0.2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pair_expr_tables.txt'))
    ap.add_argument('--overwrite', action='store_true')
    args = ap.parse_args()
    case = lj_fluid(32)
    n = len(case['positions'])
    rc = 2.5 * float(case['sigma'][0])
    kind = (np.arange(n) % 2).astype(np.float64)
    rows = PER_TYPE[kind.astype(int)]
    a, b, c = PER_TYPE[:, 0], PER_TYPE[:, 1], PER_TYPE[:, 2]
    matrices = [np.sqrt(np.outer(a, a)), 0.5 * (b[:, None] + b[None, :]), np.sqrt(np.outer(c, c))]
    lo, hi = 0.5 * float(case['sigma'][0]), rc
    knots = np.linspace(lo, hi, 901)
    ctx = B.HipContext(n, case['box'])
    x = torch.as_tensor(case['positions'], dtype=torch.float64, device='cuda')
    desc = B.pair_desc(B.PAIR_EXPR, rc)
    forces, programs = {}, {}
    programs['mixing'] = X.compile_pair(MIXING, ['A', 'B', 'C'], [])
    forces['mixing'] = ctx.pair_expr_create(desc, programs['mixing'].code, programs['mixing'].consts, [], rows[:, 0], rows[:, 1], rows[:, 2], skin=args.skin)
    programs['tables'] = X.compile_pair(TABLES, ['t'], [], {k: ('Discrete2D', 2) for k in 'ABC'})
    forces['tables'] = ctx.pair_expr_create(desc, programs['tables'].code, programs['tables'].consts, [], kind, None, None, skin=args.skin)
    ctx.pair_expr_set_tables(forces['tables'], [(T.DISCRETE2D, 2, 2, 0.0, 0.0, m.T.reshape(-1)) for m in matrices])
    programs['closed'] = X.compile_pair(CLOSED, [], [])
    forces['closed'] = ctx.pair_expr_create(desc, programs['closed'].code, programs['closed'].consts, [], None, None, None, skin=args.skin)
    programs['spline'] = X.compile_pair(SPLINE, [], [], {'U': ('Continuous1D', 1)})
    forces['spline'] = ctx.pair_expr_create(desc, programs['spline'].code, programs['spline'].consts, [], None, None, None, skin=args.skin)
    values = 1e5 * np.exp(-30.0 * knots) - 3e-3 / knots ** 6
    ctx.pair_expr_set_tables(forces['spline'], [(T.CONTINUOUS1D, 901, 1, lo, hi, T.spline_coefficients(values, lo, hi).reshape(-1))])
    out = {k: torch.zeros((n, 3), dtype=torch.float64, device='cuda') for k in forces}
    for k, fid in forces.items():
        for _ in range(3):
            ctx.force_eval(fid, x, out[k])
    us = {k: [] for k in forces}
    for _ in range(args.rounds):
        for k, fid in forces.items():
            ctx.profile_enable(True, only=fid)
            for _ in range(args.reps):
                ctx.force_eval(fid, x, out[k])
            ctx.synchronize()
            count, ms = ctx.profile_read(fid)
            ctx.profile_enable(False)
            us[k].append(1e3 * ms / count)
    ctx.check()
    f = {k: v.cpu().numpy() for k, v in out.items()}
    mean = {k: float(np.mean(v)) for k, v in us.items()}

    def line(k, text):
        return '%-7s %-52s %3d words: %8.1f us (rounds %s)' % (k, text, len(programs[k].code), mean[k], ' '.join('%.1f' % t for t in us[k]))
    lines = [
        'tabulated functions in the pair-expression kernel, config C2 (%d atoms, rc = %.3f nm, Verlet buffer %.2f nm), force only' % (n, rc, args.skin),
        'kernel revision %s, %d rounds of %d launches each, in turn, HIP events around the pair kernel; %d list entries, %d lanes per atom' %
        (B.kernel_revision(), args.rounds, args.reps, ctx.pair_stats(forces['mixing'])['n_list_pairs'], ctx.pair_stats(forces['mixing'])['lanes_per_atom']),
        line('mixing', MIXING), line('tables', TABLES),
        'ratio three Discrete2DFunction tables / mixing rules: %.3f   (max |dF| = %.2e of max |F| = %.4g)' %
        (mean['tables'] / mean['mixing'], np.abs(f['tables'] - f['mixing']).max() / np.abs(f['mixing']).max(), np.abs(f['mixing']).max()),
        line('closed', CLOSED), line('spline', SPLINE + ', Continuous1DFunction of 901 knots on [%.3f, %.3f]' % (lo, hi)),
        'ratio Continuous1DFunction / closed form: %.3f   (max |dF| = %.2e of max |F| = %.4g: the spline\'s interpolation error)' %
        (mean['spline'] / mean['closed'], np.abs(f['spline'] - f['closed']).max() / np.abs(f['closed']).max(), np.abs(f['closed']).max()),
    ]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w' if args.overwrite else 'a') as fh:
        fh.write('\n'.join(lines) + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
