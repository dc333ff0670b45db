"""What one evaluation of an RMSDForce (csrc/rmsd.hip, AMM_FORCE_RMSD) costs on its two paths, and where they cross: all N particles
of a context selected, the reference an anisotropic blob, the positions its rigid image plus 0.05 nm of noise
(tests/rmsd_cases.py), N = 64, 1 024, 16 384 and 98 304 and, with --crossover, the sizes in between.
  one block    option rmsd_blocks = 1: one launch of one block of 1 024 lanes;
  blocks       rmsd_blocks = max(2, ceil(N / 1024)): three launches of that many blocks of 256 lanes;
  restraint    for scale, what a user would otherwise reach for: a CustomExternalForce harmonic position restraint
               0.5*k*((x-x0)^2+(y-y0)^2+(z-z0)^2) on the same atoms (csrc/term_expr.hip), in the same run.
Forces + energy, HIP events on the launch stream around --reps evaluations after a warm-up, every measurement taken --rounds times
(the median is reported, the spread is the noise); the two paths' energies are printed next to each other.

    python scripts/rmsd_cost.py [--reps 500] [--rounds 5] [--sizes 64,1024,16384,98304] [--crossover 2048,4096,8192] [--out profiles/rmsd_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default='64,1024,16384,98304')
    ap.add_argument('--crossover', default='2048,4096,8192')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rmsd_cost.txt'))
    args = ap.parse_args()
    sizes = sorted({int(s) for s in (args.sizes + ',' + args.crossover).split(',') if s})
    import torch
    import rmsd_cases as RC
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    assert torch.cuda.is_available(), 'rmsd_cost.py measures on the GPU'

    def timed(ctx, fid, x, n):
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        e = torch.zeros(1, dtype=torch.float64, device='cuda')
        for _ in range(5):
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
        return float(np.median(us)), min(us), max(us), e.item() / (5 + args.rounds * args.reps)

    def show(t):
        return '%8.2f us  (lowest %.2f, highest %.2f)' % (t[0], t[1], t[2])

    lines = ['RMSDForce (csrc/rmsd.hip), all N particles selected, forces + energy, kernel revision %s' % B.kernel_revision(),
             '%d evaluations per measurement after a warm-up of 5, HIP events on the stream; median of %d rounds, the spread is the noise' % (
                 args.reps, args.rounds)]
    prog = X.compile_term('0.5*k*((x-x0)^2+(y-y0)^2+(z-z0)^2)', ('x', 'y', 'z'), ['k', 'x0', 'y0', 'z0'], [])
    crossing = []
    for n in sizes:
        ref = RC.blob(n, 1000 + n)
        pos = RC.displaced(ref, n, 0.05)
        x = torch.as_tensor(pos, dtype=torch.float64, device='cuda')
        ctx = B.HipContext(n, None)
        everyone = list(range(n))
        ctx.set_option('rmsd_blocks', 1)
        one = ctx.rmsd_create(everyone, ref)
        blocks = max(2, (n + 1023) // 1024)
        ctx.set_option('rmsd_blocks', blocks)
        many = ctx.rmsd_create(everyone, ref)
        ctx.set_option('rmsd_blocks', 0)
        chosen = ctx.rmsd_stats(ctx.rmsd_create(everyone, ref))['blocks']
        rows = np.full((n, 4), -1, dtype=np.int32)
        rows[:, 0] = np.arange(n)
        restraint = ctx.term_expr_create(B.TERM_EXTERNAL, prog.code, prog.consts, [], rows,
                                         np.stack([np.full(n, 1000.0), ref[:, 0], ref[:, 1], ref[:, 2]]))
        t_one, t_many, t_res = timed(ctx, one, x, n), timed(ctx, many, x, n), timed(ctx, restraint, x, n)
        s_one, s_many = ctx.rmsd_stats(one), ctx.rmsd_stats(many)
        ctx.close()
        crossing.append((n, t_one[0], t_many[0]))
        lines += ['N = %d (rmsd_blocks = 0 takes %s)' % (n, 'the one block' if chosen == 1 else '%d blocks' % chosen),
                  '    one block  (%d launch)            : ' % s_one['launches_per_eval'] + show(t_one) + '  rmsd = %.15g nm' % t_one[3],
                  '    %4d blocks (%d launches)          : ' % (s_many['blocks'], s_many['launches_per_eval']) + show(t_many) + '  rmsd = %.15g nm' % t_many[3],
                  '    harmonic position restraint        : ' + show(t_res) + '  (CustomExternalForce on the same atoms, term_expr.hip)']
        print('\n'.join(lines[-4:]), flush=True)
    faster = [n for n, a, b in crossing if b < a]
    lines.append('the blocks are faster than the one block at N = %s' % (', '.join(str(n) for n in faster) if faster else 'none of these sizes'))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
