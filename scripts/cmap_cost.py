"""What the CMAP kernels (csrc/cmap.hip, AMM_FORCE_CMAP) cost: HIP events on the launch stream around --reps force-only evaluations
after a warm-up, every measurement taken --rounds times (the spread is the run-to-run noise).

  1. 100, 1 000 and 100 000 CMAP terms (k .. k+3, k+1 .. k+4) with one random 24 x 24 map on a helix, next to twice as many
     AMM_TORSION_PERIODIC terms (csrc/bonded.hip) on the same atoms -- the two dihedrals of every term -- in the same run.
  2. 4 steps of RESPA [4, 2, 1] on the 1 536-atom flexible water box with 256 CMAP terms in the innermost group, against the same
     System without them: host clock around integrator.step(4) ending in a synchronise.  The group that holds the CMAP force leaves
     the fused inner loop (it is evaluated member by member); the difference is that plus the two launches per evaluation.

    python scripts/cmap_cost.py [--reps 50] [--rounds 5] [--out profiles/cmap_cost.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 24


def helix(n):
    """n atoms on a helix (0.15 nm between neighbours, no three of them collinear) with a little noise: a chain without a box."""
    t = np.arange(n)
    x = np.stack([0.1 * np.cos(1.1 * t), 0.1 * np.sin(1.1 * t), 0.11 * t], axis=1)
    return x + np.random.default_rng(2024).normal(scale=0.005, size=x.shape)


def main():
    import torch
    import atomsmm_amd as atomsmm
    from atomsmm_amd import backend as B
    from atomsmm_amd import openmm, unit
    from atomsmm_amd import tables as T
    from atomsmm_amd.testing import system_from_arrays, tip3p_box
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cmap_cost.txt'))
    args = ap.parse_args()
    energy = np.random.default_rng(5).uniform(1.0, 3.0, SIZE * SIZE)
    coeffs = T.cmap_coefficients(SIZE, energy).reshape(-1)

    def timed(ctx, fid, x, n):
        """(median, lowest, highest) microseconds per evaluation over the rounds."""
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
        return float(np.median(us)), min(us), max(us)

    def show(t):
        return '%8.1f us  (lowest %.1f, highest %.1f of %d rounds)' % (t[0], t[1], t[2], args.rounds)

    lines = ['CMAP kernels (csrc/cmap.hip), force only, kernel revision %s' % B.kernel_revision(),
             '%d evaluations per measurement after a warm-up, HIP events on the stream; median of %d rounds, the spread is the noise' % (args.reps, args.rounds)]
    # ---- 1. the helix
    for terms in (100, 1000, 100000):
        n = terms + 4
        ctx = B.HipContext(n, None)
        x = torch.as_tensor(helix(n), dtype=torch.float64, device='cuda')
        t = np.arange(terms)
        idx = np.stack([t, t + 1, t + 2, t + 3, t + 1, t + 2, t + 3, t + 4], axis=1)
        cmap = ctx.cmap_create([SIZE], coeffs, np.zeros(terms, dtype=np.int32), idx)
        rng = np.random.default_rng(7)
        rows = np.concatenate([idx[:, :4], idx[:, 4:]])
        params = np.stack([rng.integers(1, 4, 2 * terms).astype(float), rng.uniform(0.0, 3.0, 2 * terms), rng.uniform(1.0, 10.0, 2 * terms)], axis=1)
        hand = ctx.bonded_create()
        ctx.bonded_add_terms(hand, B.TORSION_PERIODIC, rows, params)
        ctx.bonded_finalize(hand)
        t_cmap, t_hand = timed(ctx, cmap, x, n), timed(ctx, hand, x, n)
        lines += ['1. %d CMAP terms, one %d x %d map, on a helix of %d atoms' % (terms, SIZE, SIZE, n),
                  '  CMAPTorsionForce                  (cmap.hip)  : ' + show(t_cmap),
                  '  %6d AMM_TORSION_PERIODIC terms (bonded.hip): ' % (2 * terms) + show(t_hand),
                  '  ratio %.2f' % (t_cmap[0] / t_hand[0])]
        ctx.close()
    # ---- 2. RESPA with CMAP innermost
    c = tip3p_box(8)
    n_terms = 256
    k = np.arange(n_terms)
    rows = np.stack([np.zeros(n_terms, dtype=np.int64), 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3, 3 * k + 1, 3 * k + 2, 3 * k + 3, 3 * k + 4], axis=1)
    ms = {}
    for with_cmap in (False, True):
        system = atomsmm.RESPASystem(system_from_arrays(c, nonbondedMethod='CutoffPeriodic'), 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        if with_cmap:
            force = openmm.CMAPTorsionForce()
            force.addMap(SIZE, energy)
            for row in rows:
                force.addTorsion(*[int(v) for v in row])
            force.setUsesPeriodicBoundaryConditions(True)
            system.addForce(force)
        integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(1 * unit.femtoseconds)
        context = openmm.Context(system, integrator)
        context.setPositions(c['positions'] * unit.nanometers)
        context.setVelocities(c['velocities'])
        ctx = context._engine.ctx
        integrator.step(8)
        ctx.synchronize()
        took = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                integrator.step(4)
            ctx.synchronize()
            took.append(1e3 * (time.perf_counter() - t0) / args.reps)
        ctx.check()
        ms[with_cmap] = (float(np.median(took)), min(took), max(took), ctx.run_stats()['epilogues'])
    lines += ['2. 4 steps of RESPA [4, 2, 1], %d-atom flexible water box, host clock around %d x step(4) ending in a synchronise' % (len(c['positions']), args.reps)]
    for with_cmap, label in ((False, 'without CMAP'), (True, 'with %d CMAP terms in group 0' % n_terms)):
        m = ms[with_cmap]
        lines += ['  %-32s: %8.3f ms per 4 steps  (lowest %.3f, highest %.3f of %d rounds); fused inner-loop epilogues so far: %d' % (
            label, m[0], m[1], m[2], args.rounds, m[3])]
    lines += ['  difference %.3f ms per 4 steps' % (ms[True][0] - ms[False][0])]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
