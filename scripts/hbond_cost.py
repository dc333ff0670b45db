"""What one evaluation of a CustomHbondForce (csrc/hbond.hip, AMM_FORCE_HBOND) costs: a three-site water box at the density of
water with D = 2 N_mol donors (H, O, -) and A = N_mol acceptors (O, H, H), the pairs within a molecule excluded, CutoffPeriodic 0.35 nm,
the texts `distance-angle` (V = 2) and `with-dihedral` (V = 3) of tests/hbond_cases.py, N_mol = 512, 4 096 and 16 384.  Per size and
text: the time of an evaluation (forces + energy) and the surviving pairs, ns per scanned pair (D x A, both passes in the time) and
per surviving pair; the time of a CustomCompoundBondForce (csrc/compound.hip) that holds the same surviving pairs as explicit bonds
-- the cost of the interpreter and the geometry alone, without the scan --; and the time with the survivors' queue switched off
(option hbond_compact 0: the interpreter runs after every batch of 64 columns that has a survivor).  HIP events on the launch stream
around --reps evaluations after a warm-up, every measurement taken --rounds times (the median is reported, the spread is the noise).

    python scripts/hbond_cost.py [--reps 10] [--rounds 5] [--sizes 512,4096,16384] [--out profiles/hbond_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DENSITY = 33.4          # molecules per nm^3
CUTOFF = 0.35


def surviving_pairs(H, pos, donors, acceptors, excl, box, block=512):
    """tests/hbond_cases.py: survivors, block of donors by block (the D x A table of 16 384 molecules does not fit)."""
    out = []
    for lo in range(0, len(donors), block):
        local = [(d - lo, a) for d, a in excl if lo <= d < lo + block]
        out += [(d + lo, a) for d, a in H.survivors(pos, donors[lo:lo + block], acceptors, local, CUTOFF, box)]
    return out


def main():
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    import hbond_cases as H
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default='512,4096,16384')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hbond_cost.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'hbond_cost.py measures on the GPU'
    kinds_of = dict(distance=B.CVAR_DISTANCE, angle=B.CVAR_ANGLE, dihedral=B.CVAR_DIHEDRAL)

    def timed(ctx, fid, x, n):
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        e = torch.zeros(1, dtype=torch.float64, device='cuda')
        for _ in range(2):
            ctx.force_eval(fid, x, f, energy=e)
        us = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.reps):
                ctx.force_eval(fid, x, f, energy=e)
            stop.record()
            ctx.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / args.reps)
        ctx.check()
        return float(np.median(us)), min(us), max(us), e.item() / (2 + args.rounds * args.reps)

    def show(t):
        return '%10.1f us  (lowest %.1f, highest %.1f)' % (t[0], t[1], t[2])

    lines = ['CustomHbondForce (csrc/hbond.hip) on three-site water boxes, CutoffPeriodic %.2f nm, forces + energy, kernel revision %s' % (CUTOFF, B.kernel_revision()),
             '%d evaluations per measurement after a warm-up of 2, HIP events on the stream; median of %d rounds, the spread is the noise' % (args.reps, args.rounds)]
    for n_mol in [int(s) for s in args.sizes.split(',')]:
        edge = (n_mol / DENSITY) ** (1.0 / 3.0)
        box = np.full(3, edge)
        pos, donors, acceptors, excl = H.water_layout(n_mol, edge, 7)
        pairs = surviving_pairs(H, pos, donors, acceptors, excl, box)
        n, D, A = len(pos), len(donors), len(acceptors)
        x = torch.as_tensor(pos, dtype=torch.float64, device='cuda')
        lines.append('N_mol = %d: %d atoms, box edge %.3f nm, D = %d donors x A = %d acceptors = %d pairs scanned per pass, %d survive on the host (%.3f %%)' % (
            n_mol, n, edge, D, A, D * A, len(pairs), 100.0 * len(pairs) / (D * A)))
        for name in ('distance-angle', 'with-dihedral'):
            case = H.TEXTS[name]
            prog, table = X.compile_hbond(case['text'], [], [], list(case['globals']))
            kinds, slots = [kinds_of[k] for k, _ in table], [list(s) for _, s in table]
            gvalues = [case['globals'][g] for g in prog.globals_]
            results = {}
            for compact in (1, 0):
                ctx = B.HipContext(n, box)
                ctx.set_option('hbond_compact', compact)
                fid = ctx.hbond_create(prog.code, prog.consts, gvalues, kinds, slots, donors, acceptors, np.zeros((0, D)), np.zeros((0, A)), excl,
                                       rc=CUTOFF, periodic=True)
                results[compact] = timed(ctx, fid, x, n)
                stats = ctx.hbond_stats(fid)
                if compact:
                    idx = np.array([H.members_of(donors, acceptors, p) for p in pairs], dtype=np.int32).reshape(-1, 6)
                    twin = ctx.compound_create(6, prog.code, prog.consts, gvalues, kinds, slots, idx, np.zeros((0, len(idx))), periodic=True)
                    results['twin'] = timed(ctx, twin, x, n)
                ctx.close()
            t, off, twin = results[1], results[0], results['twin']
            lines += ['  %s (V = %d), %d chunks per donor row' % (name, len(table), stats['chunks']),
                      '    evaluation                          : ' + show(t) + '  E = %.12g, %d surviving pairs (host: %d)' % (t[3], stats['survivors'], len(pairs)),
                      '    per scanned pair (D x A)            : %10.4f ns' % (1e3 * t[0] / (D * A)),
                      '    per surviving pair                  : %10.2f ns' % (1e3 * t[0] / max(len(pairs), 1)),
                      '    the same pairs as explicit bonds    : ' + show(twin) + '  E = %.12g (compound.hip: %.2f ns per bond)' % (twin[3], 1e3 * twin[0] / max(len(pairs), 1)),
                      '    survivors\' queue off (hbond_compact 0): ' + show(off) + '  E = %.12g, %.2f times the time with the queue' % (off[3], off[0] / t[0])]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
