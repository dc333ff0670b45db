"""What one evaluation of a GayBerneForce (csrc/gayberne.hip, AMM_FORCE_GAYBERNE) costs: a fluid of uniaxial ellipsoids (diameters
0.5 x 0.3 x 0.3 nm, sigma 0.3 nm) on a jittered cubic lattice of spacing 0.55 nm with random axes, each with one marker atom 0.1 nm
behind its centre, CutoffPeriodic 1.0 nm, at N = 512, 4 096 and 32 768 ellipsoids.  Per size: the time of an evaluation (forces +
energy, its four launches), ns per tested ordered pair (N (N - 1): every pair is met from both sides) and per surviving pair; and, as
a yardstick, the time of the Lennard-Jones NonbondedForce (csrc/pair.hip, neighbour list with the default Verlet buffer) on the
same centres with the same cutoff.  HIP events on the launch stream around --reps evaluations after a warm-up, every measurement
taken --rounds times (the median is reported, the spread is the noise).

    python scripts/gayberne_cost.py [--reps 10] [--rounds 5] [--sizes 512,4096,32768] [--out profiles/gayberne_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPACING, JITTER, CUTOFF = 0.55, 0.03, 1.0
SIGMA, EPS = 0.3, 1.5
SHAPE = (0.5, 0.3, 0.3, 1.0, 2.0, 2.0)


def fluid(n, seed):
    """(force, positions [2 n][3], box): particle 2 k is the marker of ellipsoid 2 k + 1."""
    from atomsmm_amd import openmm
    rng = np.random.default_rng(seed)
    side = int(round(n ** (1.0 / 3.0)))
    assert side ** 3 == n, 'sizes are cubes'
    grid = np.array([(a, b, c) for a in range(side) for b in range(side) for c in range(side)], dtype=np.float64)
    centres = (grid + 0.5) * SPACING + rng.uniform(-JITTER, JITTER, size=(n, 3))
    axes = rng.normal(size=(n, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    pos = np.empty((2 * n, 3))
    pos[0::2] = centres - 0.1 * axes
    pos[1::2] = centres
    force = openmm.GayBerneForce()
    for k in range(n):
        force.addParticle(SIGMA, 0.0, -1, -1, SIGMA, SIGMA, SIGMA, 1.0, 1.0, 1.0)
        force.addParticle(SIGMA, EPS, 2 * k, -1, *SHAPE)
    return force, pos, np.full(3, side * SPACING)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default='512,4096,32768')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gayberne_cost.txt'))
    args = ap.parse_args()
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import engine as E
    assert torch.cuda.is_available(), 'gayberne_cost.py measures on the GPU'

    def timed(ctx, fid, x, n):
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        e = torch.zeros(1, dtype=torch.float64, device='cuda')
        for _ in range(3):
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
        return float(np.median(us)), min(us), max(us), e.item() / (3 + args.rounds * args.reps)

    def show(t):
        return '%12.1f us  (lowest %.1f, highest %.1f)' % (t[0], t[1], t[2])

    lines = ['GayBerneForce (csrc/gayberne.hip): uniaxial ellipsoids %.1f x %.1f x %.1f nm with a marker atom each, lattice spacing %.2f nm, '
             'CutoffPeriodic %.1f nm, forces + energy, kernel revision %s' % (SHAPE[0], SHAPE[1], SHAPE[2], SPACING, CUTOFF, B.kernel_revision()),
             '%d evaluations per measurement after a warm-up of 3, HIP events on the stream; median of %d rounds, the spread is the noise' % (
                 args.reps, args.rounds)]
    for n in [int(s) for s in args.sizes.split(',')]:
        force, pos, box = fluid(n, 1000 + n)
        tab = E.gayberne_tables(force, 2 * n)
        ctx = B.HipContext(2 * n, box)
        fid = ctx.gayberne_create(tab['active'], tab['axes'], tab['par'], tab['ex_ptr'], tab['ex_col'], tab['ex_par'], tab['rev_ptr'], tab['rev_src'],
                                  rc=CUTOFF, rs=-1.0, periodic=True)
        t = timed(ctx, fid, torch.as_tensor(pos, dtype=torch.float64, device='cuda'), 2 * n)
        stats = ctx.gayberne_stats(fid)
        ctx.close()
        # the yardstick: the same centres as Lennard-Jones particles, a context of their own
        ctx = B.HipContext(n, box)
        lj = ctx.pair_create(B.pair_desc(B.NONBONDED, CUTOFF, flags=B.COULOMB_RF), np.zeros(n), np.full(n, SIGMA), np.full(n, EPS))
        t_lj = timed(ctx, lj, torch.as_tensor(pos[1::2].copy(), dtype=torch.float64, device='cuda'), n)
        ctx.close()
        pairs = stats['survivors'] // 2
        lines += ['N = %d ellipsoids (%d particles), box edge %.2f nm, %d chunks per row: %d ordered pairs tested, %d pairs survive (%.1f per ellipsoid)' % (
                      n, 2 * n, box[0], stats['chunks'], stats['scanned'], pairs, 2.0 * pairs / n),
                  '    evaluation                          : ' + show(t) + '  E = %.12g' % t[3],
                  '    per tested ordered pair             : %12.4f ns' % (1e3 * t[0] / max(stats['scanned'], 1)),
                  '    per surviving pair                  : %12.2f ns' % (1e3 * t[0] / max(pairs, 1)),
                  '    Lennard-Jones NonbondedForce, same centres and cutoff: ' + show(t_lj) + '  E = %.12g; Gay-Berne / Lennard-Jones = %.1f' % (
                      t_lj[3], t[0] / t_lj[0])]
        print('\n'.join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
