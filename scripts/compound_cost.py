"""What the compound-bond kernels (csrc/compound.hip, AMM_FORCE_COMPOUND) cost: force-only evaluations, HIP events on the launch
stream around --reps evaluations after a warm-up, every measurement taken --rounds times (the spread is the run-to-run noise).

  1. 100 000 compound bonds with the text `k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0))` on the helix of 100 003 atoms of
     scripts/term_expr_cost.py, next to the same text as a CustomTorsionForce (csrc/term_expr.hip) and as AMM_TORSION_PERIODIC
     (csrc/bonded.hip) in the same run.  (The CustomTorsionForce figure is the one profiles/term_expr_cost.txt holds for the parent.)
  2. one bond with a 16-variable text over 8 particles (tests/compound_cases.py: 'sixteen'): 16 lanes of one block.
  3. one centroid bond `0.5*k*(distance(g1,g2)-d0)^2` between two groups of 1 000 atoms in the 98 304-atom water box, alone and as
     the single collective variable of a CustomCVForce (csrc/cv.hip).

    python scripts/compound_cost.py [--reps 50] [--rounds 5] [--out profiles/compound_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TERMS = 100000
SIXTEEN = ('kb*((distance(p1,p2)-r0)^2+(distance(p2,p3)-r0)^2+(distance(p3,p4)-r0)^2+(distance(p5,p6)-r0)^2+(distance(p7,p8)-r0)^2'
           '+0.01*(distance(p1,p8)-r0)^2)'
           ' + ka*((angle(p1,p2,p3)-t0)^2+(angle(p2,p3,p4)-t0)^2+(angle(p5,p6,p7)-t0)^2+(angle(p6,p7,p8)-t0)^2)'
           ' + kd*(cos(dihedral(p1,p2,p3,p4)-phi)+cos(2*dihedral(p5,p6,p7,p8)))'
           ' + kx*((x8-x1-dx)^2+(y8-y0)^2+(z8-z0)^2)')


def helix(n):
    """n atoms on a helix (0.15 nm between neighbours, no three of them collinear) with a little noise: a chain without a box."""
    t = np.arange(n)
    x = np.stack([0.1 * np.cos(1.1 * t), 0.1 * np.sin(1.1 * t), 0.11 * t], axis=1)
    return x + np.random.default_rng(2024).normal(scale=0.005, size=x.shape)


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    from atomsmm_amd.testing.synthetic import tip3p_box
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--nside', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'compound_cost.txt'))
    args = ap.parse_args()
    kinds_of = dict(x=B.CVAR_X, y=B.CVAR_Y, z=B.CVAR_Z, distance=B.CVAR_DISTANCE, angle=B.CVAR_ANGLE, dihedral=B.CVAR_DIHEDRAL)

    def compound(ctx, text, n_slots, prefix, names, gvalues, idx, params, periodic=False, groups=None):
        prog, table = X.compile_compound(text, n_slots, prefix, names, list(gvalues))
        fid = ctx.compound_create(n_slots, prog.code, prog.consts, [gvalues[g] for g in prog.globals_], [kinds_of[k] for k, _ in table],
                                  [list(s) for _, s in table], idx, params, periodic=periodic, groups=groups)
        return fid, len(prog.code), len(table)

    def timed(ctx, fid, x, n):
        """(median, lowest, highest) microseconds per evaluation over the rounds, and the forces."""
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        for _ in range(3):
            ctx.force_eval(fid, x, f)
        us = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.reps):
                ctx.force_eval(fid, x, f)
            stop.record()
            ctx.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / args.reps)
        ctx.check()
        return (float(np.median(us)), min(us), max(us)), f.cpu().numpy()

    def show(t):
        return '%8.1f us  (lowest %.1f, highest %.1f of %d rounds)' % (t[0], t[1], t[2], args.rounds)

    lines = ['compound-bond kernels (csrc/compound.hip), force only, kernel revision %s' % B.kernel_revision(),
             '%d evaluations per measurement after a warm-up, HIP events on the stream; median of %d rounds, the spread is the noise' % (args.reps, args.rounds)]
    # ---- 1. the helix
    n = TERMS + 3
    rng = np.random.default_rng(7)
    ctx = B.HipContext(n, None)
    x = torch.as_tensor(helix(n), dtype=torch.float64, device='cuda')
    t = np.arange(TERMS)
    rows = np.stack([t, t + 1, t + 2, t + 3], axis=1)
    params = np.stack([rng.integers(1, 4, TERMS).astype(float), rng.uniform(0.0, 3.0, TERMS), rng.uniform(1.0, 10.0, TERMS)], axis=1)
    cb, words, _ = compound(ctx, 'k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0))', 4, 'p', ['n', 't0', 'k'], {}, rows, params.T)
    prog = X.compile_term('k*(1+cos(n*theta-theta0))', ('theta',), ['n', 'theta0', 'k'], [])
    generic = ctx.term_expr_create(B.TERM_TORSION, prog.code, prog.consts, [], rows.astype(np.int32), params.T)
    hand = ctx.bonded_create()
    ctx.bonded_add_terms(hand, B.TORSION_PERIODIC, rows, params)
    ctx.bonded_finalize(hand)
    got = {label: timed(ctx, fid, x, n) for label, fid in (('hand', hand), ('term', generic), ('compound', cb))}
    a = got['hand'][1]
    lines += ['1. %d torsions `k*(1+cos(n*dihedral(p1,p2,p3,p4)-t0))` (%d code words) on a helix of %d atoms' % (TERMS, words, n),
              '  AMM_TORSION_PERIODIC   (bonded.hip)   : ' + show(got['hand'][0]),
              '  CustomTorsionForce     (term_expr.hip): ' + show(got['term'][0]),
              '  CustomCompoundBondForce (compound.hip): ' + show(got['compound'][0]),
              '  ratios to the hand-written kind: %.2f (term expression), %.2f (compound bond);  max |dF| against it: %.3e, %.3e of max |F| = %.6g' % (
                  got['term'][0][0] / got['hand'][0][0], got['compound'][0][0] / got['hand'][0][0], np.abs(got['term'][1] - a).max(),
                  np.abs(got['compound'][1] - a).max(), np.abs(a).max())]
    # ---- 2. one bond, sixteen variables (the same context: n atoms, the gather walks all of them)
    names = ['kb', 'r0', 'ka', 't0', 'kd', 'phi', 'kx', 'dx']
    one, words, n_vars = compound(ctx, SIXTEEN, 8, 'p', names, dict(y0=1.0, z0=2.0), np.arange(8).reshape(1, 8) * 3,
                                  np.array([[300.0, 0.4, 50.0, 1.9, 5.0, 0.3, 10.0, 0.1]]).T)
    lines += ['2. one bond over 8 particles, %d variables, %d code words (n = %d atoms: the gather writes every row)' % (n_vars, words, n),
              '  CustomCompoundBondForce (compound.hip): ' + show(timed(ctx, one, x, n)[0])]
    ctx.close()
    # ---- 3. one centroid bond in the water box
    c = tip3p_box(args.nside)
    n = len(c['positions'])
    ctx = B.HipContext(n, c['box'])
    x = torch.as_tensor(c['positions'], dtype=torch.float64, device='cuda')
    members = np.concatenate([np.arange(0, 1000), np.arange(50000, 51000)]).astype(np.int32)
    groups = (np.array([0, 1000, 2000], dtype=np.int32), members, np.asarray(c['mass'])[members])
    alone, words, _ = compound(ctx, '0.5*k*(distance(g1,g2)-d0)^2', 2, 'g', [], dict(k=100.0, d0=1.0), [[0, 1]], np.zeros((0, 1)), periodic=True, groups=groups)
    inner, _, _ = compound(ctx, 'distance(g1,g2)', 2, 'g', [], {}, [[0, 1]], np.zeros((0, 1)), periodic=True, groups=groups)
    outer = X.compile_cv('0.5*k*(d-d0)^2', ['d'], [], ['k', 'd0'])
    cv = ctx.cv_create([inner], 0, outer.code, outer.consts, [dict(k=100.0, d0=1.0)[g] for g in outer.globals_])
    t_alone, f_alone = timed(ctx, alone, x, n)
    t_cv, f_cv = timed(ctx, cv, x, n)
    lines += ['3. one centroid bond between two groups of 1000 atoms in the water box of %d atoms (three launches: centres, bond, spread; the CV force adds its combine)' % n,
              '  CustomCentroidBondForce alone         : ' + show(t_alone),
              '  as the one CV of a CustomCVForce      : ' + show(t_cv),
              '  max |dF| between the two: %.3e of max |F| = %.6g' % (np.abs(f_alone - f_cv).max(), np.abs(f_alone).max())]
    ctx.close()
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
