"""What one evaluation of the generalized-Born force (csrc/gb.hip, AMM_FORCE_GB) costs next to the `nocutoff` NONBONDED evaluation of
csrc/free.hip on the same atoms, in the same process: force-only evaluations, HIP events on the launch stream around --reps evaluations
after a warm-up, every measurement taken --rounds times (the spread is the run-to-run noise).  Sizes: 1 527 atoms (the first 509 waters
of q-SPC-FW), 4 608 (the box three times in a row) and 32 768 (the box replicated on a 3 x 3 x 3 grid, cut at the size limit).  The
per-pass kernel times come from a profiled run of a few evaluations afterwards (torch.profiler: device durations by kernel name).

    python scripts/gb_cost.py [--reps 20] [--rounds 5] [--out profiles/gb_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PASSES = ('k_gb_born', 'k_gb_pair', 'k_gb_chain')
# what the passes carry per pair (csrc/gb.hip), for whoever reads the ratio: it is not the pass count
NOTE = ['reading the ratio: three passes over all pairs, but not three Coulomb + LJ passes.  Per pair, k_gb_pair takes an exp and an rsqrt',
        '(about the cost of the NONBONDED pass), k_gb_born a square root, a division and one fp64 logarithm, k_gb_chain a square root, a',
        'division and two logarithms (one per role of the atom).  The fp64 log is a software routine of about as many instructions as the',
        'whole Coulomb + LJ pair: the chain pass, then the Born pass, are where the time above the pass count goes.']


def replicated(spcfw, n):
    """The first n atoms of the fixture box replicated on a grid (x fastest): positions, charges, masses."""
    L = spcfw['box']
    copies = -(-n // len(spcfw['positions']))
    side = int(np.ceil(copies ** (1.0 / 3.0)))
    shifts = [np.array([i, j, k]) * L for k in range(side) for j in range(side) for i in range(side)][:copies]
    pos = np.concatenate([spcfw['positions'] + s for s in shifts])[:n]
    return dict(positions=pos, charge=np.tile(spcfw['charge'], copies)[:n], mass=np.tile(spcfw['mass'], copies)[:n],
                sigma=np.tile(spcfw['sigma'], copies)[:n], epsilon=np.tile(spcfw['epsilon'], copies)[:n])


def main():
    import torch
    from atomsmm_amd import backend as B
    import gb_cases as G
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default='1527,4608,32768')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gb_cost.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'gb_cost.py measures on the GPU'
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'q-SPC-FW.npz'))
    spcfw = {k: d[k] for k in d.files}

    def timed(ctx, fid, x, n, reps):
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        for _ in range(3):
            ctx.force_eval(fid, x, f)
        us = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                ctx.force_eval(fid, x, f)
            stop.record()
            ctx.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / reps)
        ctx.check()
        return float(np.median(us)), min(us), max(us)

    def per_pass(ctx, fid, x, n, reps):
        """Mean device microseconds per launch of each pass (None: the profiler saw no such kernel)."""
        from torch.profiler import ProfilerActivity, profile
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                ctx.force_eval(fid, x, f)
            ctx.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in PASSES:
                if name in ev.key:
                    total = getattr(ev, 'device_time_total', None)
                    if total is None:
                        total = getattr(ev, 'cuda_time_total', 0.0)
                    out[name] = out.get(name, 0.0) + total / reps
        return out

    def show(t):
        return '%10.1f us  (lowest %.1f, highest %.1f of %d rounds)' % (t[0], t[1], t[2], args.rounds)

    lines = ['generalized-Born force (csrc/gb.hip) against the nocutoff NONBONDED force (csrc/free.hip), force only, kernel revision %s'
             % B.kernel_revision(),
             '%d evaluations per measurement (fewer at 32768 atoms: see there) after a warm-up, HIP events on the stream; median of %d '
             'rounds, the spread is the noise' % (args.reps, args.rounds)]
    for n in [int(s) for s in args.sizes.split(',')]:
        c = replicated(spcfw, n)
        R, S = G.radii_by_mass(c['mass'])
        reps = args.reps if n <= 8192 else max(3, args.reps // 4)
        ctx = B.HipContext(n, None)
        x = torch.as_tensor(c['positions'], dtype=torch.float64, device='cuda')
        gb = ctx.gb_create(c['charge'], R, S)
        nb = ctx.pair_create(B.pair_desc(B.NONBONDED, 0.0, flags=B.FREE_SPACE), c['charge'], c['sigma'], c['epsilon'])
        t_nb = timed(ctx, nb, x, n, reps)
        t_gb = timed(ctx, gb, x, n, reps)
        passes = per_pass(ctx, gb, x, n, min(reps, 5))
        lanes = ctx.pair_stats(nb)['lanes_per_atom']
        lines += ['%d atoms (%d lanes per row, %d evaluations per measurement)' % (n, lanes, reps),
                  '  NONBONDED nocutoff (free.hip): ' + show(t_nb),
                  '  GBSAOBCForce       (gb.hip)  : ' + show(t_gb),
                  '  ratio GB / NONBONDED: %.2f' % (t_gb[0] / t_nb[0])]
        if passes:
            lines.append('  per pass (device time per launch): ' + ', '.join(
                '%s %.1f us' % (name, passes[name]) if name in passes else '%s not seen' % name for name in PASSES))
        else:
            lines.append('  per pass: not measured (the profiler reported no device activity)')
        ctx.close()
    lines += NOTE
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
