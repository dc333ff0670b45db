"""What one evaluation of a CustomGBForce (csrc/custom_gb.hip, AMM_FORCE_CUSTOM_GB) costs next to the hand-written GBSAOBCForce
(csrc/gb.hip) on the same atoms, in the same process: the model `obc2-text` of tests/custom_gb_cases.py -- OBC2 as texts, the same
numbers as the hand-written kernels give -- forces + energy, HIP events on the launch stream around --reps evaluations after a warm-up,
every measurement taken --rounds times (the median is reported, the spread is the run-to-run noise).  Sizes: 1 527 atoms (the first 509
waters of q-SPC-FW) and 4 608 (gb_cases.d4608: the box three times in a row).  The per-pass kernel times come from a profiled run of a
few evaluations afterwards (torch.profiler: device durations by kernel name).

    python scripts/custom_gb_cost.py [--reps 20] [--rounds 5] [--out profiles/custom_gb_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PASSES = {'text': ('k_cgb_value', 'k_cgb_atom', 'k_cgb_energy', 'k_cgb_chain'), 'hand': ('k_gb_born', 'k_gb_pair', 'k_gb_chain')}
NOTE = ['reading the ratio: per ordered pair the text model runs the interpreter five times -- the integral I once (74 words: a max, an abs,',
        'a step, a log, five divisions), the pair term twice (34 words, seeded in r and in B1: an exp, a sqrt, two divisions each) and the',
        'integral twice more in the chain pass (seeded in r, the roles swapped) -- where the hand-written kernels take one division per pair',
        'and pass.  The row atom\'s parameters and values are read from global memory by every run.']


def main():
    import torch
    from atomsmm_amd import backend as B
    import custom_gb_cases as M
    import gb_cases as G
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'custom_gb_cost.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'custom_gb_cost.py measures on the GPU'
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'q-SPC-FW.npz'))
    spcfw = {k: d[k] for k in d.files}

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

    def per_pass(ctx, fid, x, n, names, reps=5):
        """Mean device microseconds per launch of each pass (missing: the profiler saw no such kernel)."""
        from torch.profiler import ProfilerActivity, profile
        f = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
        e = torch.zeros(1, dtype=torch.float64, device='cuda')
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                ctx.force_eval(fid, x, f, energy=e)
            ctx.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in names:
                if name in ev.key:
                    total = getattr(ev, 'device_time_total', None)
                    if total is None:
                        total = getattr(ev, 'cuda_time_total', 0.0)
                    out[name] = out.get(name, 0.0) + total / reps
        return out

    def show(t):
        return '%10.1f us  (lowest %.1f, highest %.1f of %d rounds)' % (t[0], t[1], t[2], args.rounds)

    lines = ['CustomGBForce obc2-text (csrc/custom_gb.hip) against GBSAOBCForce (csrc/gb.hip), forces + energy, kernel revision %s' % B.kernel_revision(),
             '%d evaluations per measurement after a warm-up of 3, HIP events on the stream; median of %d rounds, the spread is the noise'
             % (args.reps, args.rounds)]
    cases = [('1527', G.with_radii(G.d1527(spcfw))), ('4608', G.d4608(spcfw))]
    for label, c in cases:
        n = len(c['positions'])
        ctx = B.HipContext(n, None)
        x = torch.as_tensor(c['positions'], dtype=torch.float64, device='cuda')
        hand = ctx.gb_create(c['charge'], c['radius'], c['scale'])
        text = M.create_on(ctx, M.obc2_force(c))
        t_hand = timed(ctx, hand, x, n)
        t_text = timed(ctx, text, x, n)
        lines += ['%d atoms' % n,
                  '  GBSAOBCForce  (gb.hip)       : ' + show(t_hand) + '  E = %.12g' % t_hand[3],
                  '  obc2-text     (custom_gb.hip): ' + show(t_text) + '  E = %.12g' % t_text[3],
                  '  ratio text / hand-written: %.1f' % (t_text[0] / t_hand[0])]
        for which, fid in (('hand', hand), ('text', text)):
            passes = per_pass(ctx, fid, x, n, PASSES[which])
            lines.append('  per pass, %s (device time per launch): ' % which + (', '.join(
                '%s %.1f us' % (name, passes[name]) if name in passes else '%s not seen' % name for name in PASSES[which])
                if passes else 'not measured (the profiler reported no device activity)'))
        ctx.close()
    lines += NOTE
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
