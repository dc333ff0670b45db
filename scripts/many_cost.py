"""What one evaluation of a CustomManyParticleForce (csrc/manyparticle.hip, AMM_FORCE_MANY_PARTICLE) costs: one site per molecule at
the density of water (33.4 per nm^3) on a jittered grid, CutoffPeriodic --
  mW-like   the Stillinger-Weber three-body term (text `stillinger-weber` of tests/manyparticle_cases.py, V = 3),
            UniqueCentralParticle, cutoff 0.43 nm, 512, 4 096 and 32 768 particles;
  AT        the Axilrod-Teller triple-dipole term (`axilrod-teller`, V = 6), SinglePermutation, cutoff 1.0 nm, 512 and 4 096 particles
            (at 32 768 the explicit bonds of the comparison would number fifty million).
Per case: the time of an evaluation (forces + energy), the sets evaluated (amm_many_stats against the host's count), ns per set, and
the time of a CustomCompoundBondForce (csrc/compound.hip) that holds the same sets as explicit bonds of three particles -- the cost of
one interpretation per set without the neighbour scan and the enumeration; the many-particle kernel interprets every set three times,
once per owner.  HIP events on the launch stream around --reps evaluations after a warm-up, every measurement taken --rounds times
(the median is reported, the spread is the noise).  The sets are enumerated on the host with numpy; --prepare does only that and
keeps them under scripts/_cache, where a later run finds them.

    python scripts/many_cost.py [--reps 10] [--rounds 5] [--mw 512,4096,32768] [--at 512,4096] [--out profiles/many_cost.txt] [--prepare]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
CACHE = os.path.join(ROOT, 'scripts', '_cache')

DENSITY = 33.4          # particles per nm^3
CASES = dict(mw=dict(text='stillinger-weber', central=True, cutoff=0.43), at=dict(text='axilrod-teller', central=False, cutoff=1.0))


def fluid(n, seed=7):
    """(positions, box): a jittered grid at the density of water."""
    edge = (n / DENSITY) ** (1.0 / 3.0)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    rng = np.random.default_rng(seed)
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)[:n]
    return (grid + 0.5 + rng.uniform(-0.3, 0.3, (n, 3))) * (edge / side), np.full(3, edge)


def neighbour_lists(pos, box, cutoff, block=128):
    """Per particle the sorted partners inside the cutoff under the minimum image, in fp64 as lower index minus higher index."""
    n = len(pos)
    out = []
    for lo in range(0, n, block):
        d = pos[lo:lo + block, None, :] - pos[None, :, :]
        d -= box * np.rint(d / box)
        r2 = (d ** 2).sum(axis=2)
        for i in range(lo, min(lo + block, n)):
            near = np.nonzero(r2[i - lo] < cutoff * cutoff)[0]
            out.append(near[near != i])
    return out


def enumerate_sets(pos, box, cutoff, central):
    """[sets][3] as (p1, p2, p3): UniqueCentralParticle -- the centre and every pair j < k of its neighbours; SinglePermutation --
    i < j < k with all three distances inside the cutoff."""
    nbr = neighbour_lists(pos, box, cutoff)
    pairs_of = {}
    out = []
    for i, near in enumerate(nbr):
        if not central:
            near = near[near > i]
        m = len(near)
        if m < 2:
            continue
        if m not in pairs_of:
            pairs_of[m] = np.triu_indices(m, 1)
        a, b = pairs_of[m]
        j, k = near[a], near[b]
        if not central:
            d = pos[j] - pos[k]
            d -= box * np.rint(d / box)
            keep = (d ** 2).sum(axis=1) < cutoff * cutoff
            j, k = j[keep], k[keep]
        out.append(np.stack([np.full(len(j), i), j, k], axis=1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 3), dtype=np.int32)


def sets_of(kind, n):
    path = os.path.join(CACHE, 'many_sets_%s_%d.npy' % (kind, n))
    pos, box = fluid(n)
    if os.path.exists(path):
        return pos, box, np.load(path)
    sets = enumerate_sets(pos, box, CASES[kind]['cutoff'], CASES[kind]['central'])
    os.makedirs(CACHE, exist_ok=True)
    np.save(path, sets)
    return pos, box, sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--mw', default='512,4096,32768')
    ap.add_argument('--at', default='512,4096')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'many_cost.txt'))
    ap.add_argument('--prepare', action='store_true')
    args = ap.parse_args()
    todo = [('mw', int(s)) for s in args.mw.split(',') if s] + [('at', int(s)) for s in args.at.split(',') if s]
    if args.prepare:
        for kind, n in todo:
            print(kind, n, len(sets_of(kind, n)[2]), 'sets', flush=True)
        return
    import torch
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    import manyparticle_cases as M
    assert torch.cuda.is_available(), 'many_cost.py measures on the GPU'
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

    lines = ['CustomManyParticleForce (csrc/manyparticle.hip), one site per molecule at %.1f per nm^3, CutoffPeriodic, forces + energy, kernel revision %s' % (
                 DENSITY, B.kernel_revision()),
             '%d evaluations per measurement after a warm-up of 2, HIP events on the stream; median of %d rounds, the spread is the noise' % (args.reps, args.rounds)]
    for kind, n in todo:
        case, text = CASES[kind], M.TEXTS[CASES[kind]['text']]
        pos, box, sets = sets_of(kind, n)
        prog, table = X.compile_many_particle(text['text'], 3, [], list(text['globals']))
        kinds, slots = [kinds_of[k] for k, _ in table], [list(s) for _, s in table]
        gvalues = [text['globals'][g] for g in prog.globals_]
        x = torch.as_tensor(pos, dtype=torch.float64, device='cuda')
        ctx = B.HipContext(n, box)
        fid = ctx.many_create(prog.code, prog.consts, gvalues, kinds, slots, np.zeros((0, n)), np.zeros(n, dtype=np.int32), 1, [0], None,
                              rc=case['cutoff'], periodic=True, central=case['central'])
        t = timed(ctx, fid, x, n)
        stats = ctx.many_stats(fid)
        twin = ctx.compound_create(3, prog.code, prog.consts, gvalues, kinds, slots, sets, np.zeros((0, len(sets))), periodic=True)
        tw = timed(ctx, twin, x, n)
        ctx.close()
        lines += ['%s, %d particles, box edge %.3f nm: %s (V = %d), %s, cutoff %.2f nm, fullest neighbour row %d of %d' % (
                      kind, n, box[0], CASES[kind]['text'], len(table), 'UniqueCentralParticle' if case['central'] else 'SinglePermutation',
                      case['cutoff'], stats['fullest'], stats['capacity']),
                  '    evaluation                          : ' + show(t) + '  E = %.12g, %d sets (host: %d)' % (t[3], stats['sets'], len(sets)),
                  '    per set                             : %10.2f ns (three interpretations each)' % (1e3 * t[0] / max(len(sets), 1)),
                  '    the same sets as explicit bonds     : ' + show(tw) + '  E = %.12g (compound.hip: %.2f ns per bond; the evaluation above takes %.2f times this)' % (
                      tw[3], 1e3 * tw[0] / max(len(sets), 1), t[0] / tw[0])]
        print('\n'.join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
