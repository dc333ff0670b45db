#!/usr/bin/env python3
"""What virtual sites cost: a step of LangevinMiddleIntegrator(300 K, 1/ps, 2 fs) on rigid TIP4P-Ew water (four sites, the M site a
ThreeParticleAverageSite) against rigid TIP3P water (three sites) -- the same 24 576 molecules on the same lattice, PME, cutoff 0.9 nm.

    python scripts/vsite_cost.py [--grid 32 32 24] [--steps 1000] [--repeats 5] [--out profiles/vsite_cost.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/vsite_cost.py --trace 200
    python scripts/vsite_cost.py --summarise OUT [--out profiles/vsite_cost.txt]          # appends the kernel table

The two models live in one process, are relaxed the same way and timed in turn (alternating windows of `--steps` steps after a warm-up
window, device events): the spread of a model's windows is what the difference between the two has to exceed.  The TIP3P box takes the
path it took before virtual sites existed (molecule rows, fused launches); the four-site box takes per-atom rows, every op on its own,
one placement per step and one spread per evaluation.  Kernel times come from a trace run of their own (--trace under rocprofv3).
Prints one JSON line; --out also writes the table."""
import argparse
import csv
import glob
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPERATURE, FRICTION, DT_FS, CUTOFF = 300.0, 1.0, 2.0, 0.9
R_OH, THETA, D_OM = 0.09572, math.radians(104.52), 0.0125
MODELS = {  # (q_O, q_H, q_M, sigma_O, eps_O)
    'tip3p': (-0.834, 0.417, None, 0.315075, 0.635968),
    'tip4pew': (0.0, 0.52422, -1.04844, 0.316435, 0.680946),
}
KERNELS = ('k_vsite_place', 'k_vsite_spread', 'k_vsite_zero')


def lattice(grid, seed=7, density=33.368):
    """O, H1, H2 of grid[0] x grid[1] x grid[2] waters on a lattice with random orientations; returns ([nmol][3][3], box)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    a = (1.0 / density) ** (1.0 / 3.0)
    axes = [(np.arange(g) + 0.5) * a for g in grid]
    centers = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)
    nmol = len(centers)
    h = np.array([[R_OH * math.sin(THETA / 2), R_OH * math.cos(THETA / 2), 0.0], [-R_OH * math.sin(THETA / 2), R_OH * math.cos(THETA / 2), 0.0]])
    q = rng.normal(size=(nmol, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)
    pos = np.empty((nmol, 3, 3))
    pos[:, 0] = centers
    pos[:, 1] = centers + R @ h[0]
    pos[:, 2] = centers + R @ h[1]
    return pos, np.array([g * a for g in grid])


def build(model, pos, box):
    """Rigid water of `model` as a System (what app.ForceField.createSystem(PME, rigidWater=True) makes), in a Simulation."""
    import numpy as np
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.openmm import app
    q_o, q_h, q_m, sigma, eps = MODELS[model]
    per = 3 if q_m is None else 4
    nmol = len(pos)
    w_h = D_OM / (2.0 * R_OH * math.cos(0.5 * THETA))
    r_hh = 2.0 * R_OH * math.sin(0.5 * THETA)
    system = openmm.System()
    nb = openmm.NonbondedForce()
    x = np.zeros((nmol, per, 3))
    x[:, :3] = pos
    if per == 4:
        x[:, 3] = (1.0 - 2.0 * w_h) * pos[:, 0] + w_h * pos[:, 1] + w_h * pos[:, 2]
    for m in range(nmol):
        b = per * m
        for mass, q, s, e in ((15.99943, q_o, sigma, eps), (1.007947, q_h, 1.0, 0.0), (1.007947, q_h, 1.0, 0.0)):
            system.addParticle(mass)
            nb.addParticle(q, s, e)
        system.addConstraint(b, b + 1, R_OH)
        system.addConstraint(b, b + 2, R_OH)
        system.addConstraint(b + 1, b + 2, r_hh)
        if per == 4:
            system.addParticle(0.0)
            nb.addParticle(q_m, 1.0, 0.0)
            system.setVirtualSite(b + 3, openmm.ThreeParticleAverageSite(b, b + 1, b + 2, 1.0 - 2.0 * w_h, w_h, w_h))
        for i in range(per):
            for j in range(i + 1, per):
                nb.addException(b + i, b + j, 0.0, 1.0, 0.0)
    system.setDefaultPeriodicBoxVectors((float(box[0]), 0, 0), (0, float(box[1]), 0), (0, 0, float(box[2])))
    nb.setNonbondedMethod(openmm.NonbondedForce.PME)
    nb.setCutoffDistance(CUTOFF)
    system.addForce(nb)
    integrator = openmm.LangevinMiddleIntegrator(TEMPERATURE * unit.kelvin, FRICTION / unit.picosecond, DT_FS * unit.femtoseconds)
    integrator.setRandomNumberSeed(11)
    simulation = app.Simulation(app.Topology(per * nmol), system, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(x.reshape(-1, 3) * unit.nanometers)
    simulation.context.setVelocitiesToTemperature(TEMPERATURE * unit.kelvin, 5)
    return simulation


def relax(simulation, nmol, max_steps, block=10):
    """Untimed: the lattice start to liquid-like water near 300 K by rescaling velocities (six degrees of freedom per rigid water)."""
    from atomsmm_amd import unit
    eng = simulation.context._engine
    dof, kB = 6 * nmol, unit.BOLTZMANN_CONSTANT_kB._value
    done = calm = 0
    T = float('nan')
    while done < max_steps and calm < 5:
        simulation.step(block)
        done += block
        T = 2.0 * simulation.context.getState(getEnergy=True).getKineticEnergy()._value / (dof * kB)
        eng.v.mul_((TEMPERATURE / T) ** 0.5)
        calm = calm + 1 if T < 1.04 * TEMPERATURE else 0
    return done, T


def summarise(directory):
    path = glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True)[0]
    rows = list(csv.DictReader(open(path)))
    lines = ['kernel times of the four-site box (rocprofv3 --kernel-trace --stats, a run of its own):',
             '%-28s %8s %12s %10s %10s' % ('kernel', 'calls', 'average us', 'min us', 'max us')]
    for name in KERNELS:
        r = next((r for r in rows if name in r['Name']), None)
        if r is None:
            lines.append('%-28s not in the trace' % name)
        else:
            lines.append('%-28s %8s %12.2f %10.2f %10.2f' % (name, r['Calls'], float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    mine = sum(float(r['TotalDurationNs']) for r in rows if any(name in r['Name'] for name in KERNELS))
    lines.append('their share of all kernel time in the trace: %.3f %%' % (100.0 * mine / total))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--grid', type=int, nargs=3, default=[32, 32, 24], help='waters per box edge (32 32 24 -> 24 576 waters)')
    ap.add_argument('--steps', type=int, default=1000, help='steps per timed window')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--relax', type=int, default=600)
    ap.add_argument('--trace', type=int, default=0, metavar='STEPS', help='only the four-site box, this many steps after the warm-up (for a kernel trace)')
    ap.add_argument('--summarise', metavar='DIR', help='print the virtual-site rows of a kernel trace')
    ap.add_argument('--out', help='write (--summarise: append) the table here')
    args = ap.parse_args()
    if args.summarise:
        lines = summarise(args.summarise)
        print('\n'.join(lines))
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write('\n' + '\n'.join(lines) + '\n')
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('vsite_cost.py measures on the GPU: none found')
    pos, box = lattice(args.grid)
    nmol = len(pos)
    models = ['tip4pew'] if args.trace else ['tip3p', 'tip4pew']
    sims, notes = {}, {}
    for model in models:
        sims[model] = build(model, pos, box)
        notes[model] = dict(relax=relax(sims[model], nmol, args.relax))
    for model in models:                          # warm-up: every program compiled, every list built
        sims[model].step(args.steps)
    if args.trace:
        sims['tip4pew'].step(args.trace)
        torch.cuda.synchronize()
        sims['tip4pew'].context._engine._check()
        return
    per_step = {}
    for model in models:
        eng = sims[model].context._engine
        before, sched = eng.ctx.vsite_stats(), eng.ctx.run_stats()['scheduled']
        sims[model].step(20)
        after = eng.ctx.vsite_stats()
        pid = eng.pair_force_ids(0)[0]
        per_step[model] = dict(places=(after['places'] - before['places']) / 20.0, spreads=(after['spreads'] - before['spreads']) / 20.0,
                               vsite_launches=(after['launches'] - before['launches']) / 20.0,
                               ops_scheduled=(eng.ctx.run_stats()['scheduled'] - sched) / 20.0, list_kind=eng.ctx.pair_stats(pid)['list_kind'])
    torch.cuda.synchronize()
    windows = {model: [] for model in models}
    for _ in range(args.repeats):
        for model in models:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            sims[model].step(args.steps)
            stop.record()
            stop.synchronize()
            windows[model].append(start.elapsed_time(stop) / args.steps)
    out = dict(waters=nmol, box=[round(float(b), 4) for b in box], steps_per_window=args.steps, per_step=per_step, ms_per_step={})
    lines = ['scripts/vsite_cost.py: rigid water, LangevinMiddleIntegrator(300 K, 1/ps, 2 fs), PME, cutoff %.1f nm, %d waters, box %s nm' %
             (CUTOFF, nmol, ' x '.join('%.3f' % b for b in box)),
             '%d windows of %d steps per model, alternating, device events; relaxed %s' %
             (args.repeats, args.steps, ', '.join('%s %d steps to %.0f K' % (m, notes[m]['relax'][0], notes[m]['relax'][1]) for m in models)),
             '', '%-8s %6s %10s %10s %10s   %s' % ('model', 'atoms', 'median ms', 'min ms', 'max ms', 'per step')]
    for model in models:
        w = sorted(windows[model])
        out['ms_per_step'][model] = dict(median=w[len(w) // 2], min=w[0], max=w[-1], windows=windows[model])
        sims[model].context._engine._check()
        p = per_step[model]
        lines.append('%-8s %6d %10.4f %10.4f %10.4f   %.0f ops scheduled, list kind %d, %.0f placements, %.0f spreads, %.0f virtual-site launches' %
                     (model, sims[model].context._engine.n, w[len(w) // 2], w[0], w[-1], p['ops_scheduled'], p['list_kind'], p['places'], p['spreads'],
                      p['vsite_launches']))
    if len(models) == 2:
        ratio = out['ms_per_step']['tip4pew']['median'] / out['ms_per_step']['tip3p']['median']
        out['ratio'] = ratio
        lines.append('four-site / three-site (medians): %.3f' % ratio)
    print('\n'.join(lines), file=sys.stderr)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
