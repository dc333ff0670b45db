"""What a DrudeForce evaluation (csrc/drude.hip, AMM_FORCE_DRUDE) and a DrudeLangevinIntegrator step (AMM_OP_DRUDE_STEP) cost on
rigid polarizable water (atomsmm_amd.testing.swm4_box: O, D, H1, H2, M per molecule) at 512, 4 096 and 32 768 waters, through the
library's entry points, no other force in the way.  Per size:

  force  one evaluation (forces + energy, its two launches) of the DrudeForce -- one isotropic spring per water -- and, beside it, a
         HarmonicBondForce with as many bonds on the same atoms (csrc/bonded.hip);
  step   one AMM_OP_DRUDE_STEP on a fixed force buffer (zero forces, thermal velocities, the rigid-water constraint set) and, beside
         it, AMM_OP_STOCK of kind AMM_STOCK_LANGEVIN on the same atoms and constraints.

HIP events on the launch stream around --reps evaluations or steps after a warm-up, every measurement taken --rounds times (the
median is reported, the spread is the noise).

    python scripts/drude_cost.py [--reps 20] [--rounds 5] [--sides 8,16,32] [--out profiles/drude_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, FRICTION, DRUDE_FRICTION, T, TD = 0.001, 5.0, 20.0, 300.0, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sides', default='8,16,32')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'drude_cost.txt'))
    args = ap.parse_args()
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import unit
    from atomsmm_amd.testing import swm4_box
    assert torch.cuda.is_available(), 'drude_cost.py measures on the GPU'
    kB = unit.BOLTZMANN_CONSTANT_kB._value

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')

    def measure(ctx, run):
        for _ in range(3):
            run(1)
        us = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run(args.reps)
            stop.record()
            ctx.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / args.reps)
        ctx.check()
        return float(np.median(us)), min(us), max(us)

    def show(t):
        return '%10.1f us  (lowest %.1f, highest %.1f)' % t

    lines = ['DrudeForce and DrudeLangevinIntegrator step (csrc/drude.hip) on rigid SWM4-like water (5 sites: O, D, H1, H2, M), kernel revision %s'
             % B.kernel_revision(),
             '%d evaluations / steps per measurement after a warm-up of 3, HIP events on the stream; median of %d rounds, the spread is the noise'
             % (args.reps, args.rounds)]
    for side in [int(s) for s in args.sides.split(',')]:
        case = swm4_box(side)
        n, waters = len(case['mass']), case['n_waters']
        rows = np.array(case['drude'], dtype=np.float64)
        idx, par = rows[:, :5].astype(np.int32), rows[:, 5:]

        def fresh():
            ctx = B.HipContext(n, case['box'])
            x, v = dev(case['positions']), dev(case['velocities'])
            ctx.bind_state(x, v, dev(case['mass']))
            return ctx, x, v
        # ---- the force and its yardstick
        ctx, x, v = fresh()
        f, e = torch.zeros((n, 3), dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda')
        fid = ctx.drude_create(idx, par, np.zeros((0, 2), np.int32), np.zeros(0), periodic=True)

        def eval_drude(k):
            for _ in range(k):
                ctx.force_eval(fid, x, f, energy=e)
        t_force = measure(ctx, eval_drude)
        k_spring = 138.935456 * par[:, 0] ** 2 / par[:, 1]
        bid = ctx.bonded_create()
        ctx.bonded_add_terms(bid, B.BOND_HARMONIC, idx[:, :2], np.stack([np.zeros(waters), k_spring], 1), periodic=True)
        ctx.bonded_finalize(bid)

        def eval_bonds(k):
            for _ in range(k):
                ctx.force_eval(bid, x, f, energy=e)
        t_bond = measure(ctx, eval_bonds)
        ctx.close()
        # ---- the step and its yardstick, each in a context of its own (the steps move the atoms)
        cons = case['constraints']
        pairs, dist = np.array([(c[0], c[1]) for c in cons], dtype=np.int32), np.array([c[2] for c in cons])
        steps = {}
        for name in ('drude', 'langevin'):
            ctx, x, v = fresh()
            zero = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
            ctx.bind_buffer(0, zero)
            ctx.constraints_create(pairs, dist, 1e-5)
            ctx.expr_seed(17)
            if name == 'drude':
                sid = ctx.drude_step_define(idx[:, :2], DT, FRICTION, kB * T, DRUDE_FRICTION, kB * TD, 0.0)
                op = B.Op(B.OP_DRUDE_STEP, sid, 0, 0, 0.0)
            else:
                sid = ctx.stock_define(B.STOCK_LANGEVIN, DT, FRICTION, kB * T)
                op = B.Op(B.OP_STOCK, sid, 0, 0, 0.0)
            steps[name] = measure(ctx, lambda k, ctx=ctx, op=op: ctx.run_ops([op], k))
            ctx.close()
        lines += ['%d waters (%d particles), box edge %.2f nm: %d springs, %d rigid triangles' % (waters, n, case['box'][0], waters, waters),
                  '    DrudeForce evaluation                 : ' + show(t_force),
                  '    HarmonicBondForce, same atoms         : ' + show(t_bond) + '   Drude / bonds = %.2f' % (t_force[0] / t_bond[0]),
                  '    AMM_OP_DRUDE_STEP                     : ' + show(steps['drude']),
                  '    AMM_OP_STOCK (Langevin), same atoms   : ' + show(steps['langevin']) + '   Drude / stock = %.2f'
                  % (steps['drude'][0] / steps['langevin'][0])]
        print('\n'.join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
