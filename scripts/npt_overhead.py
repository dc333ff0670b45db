#!/usr/bin/env python3
"""What a MonteCarloBarostat costs on the flagship workload (config C3: 98 304 atoms of flexible TIP3P water, RESPA [4, 2, 1] at
4 fs, the system of bench.py): ms per step with and without a barostat at `--frequency` (default 25), the extra time per attempt,
and what amm_set_box did over the timed windows (amm_box_stats).

    python scripts/npt_overhead.py [--nside 32] [--frequency 25] [--repeats 3] [--window 1.0]
    python scripts/npt_overhead.py --attempts K [--nside 32]      # nothing is timed: setup, a warm-up and K attempts

The two simulations live in one process, start from the same relaxed liquid and are timed in turn, each warmed up, `--repeats`
windows of at least `--window` seconds each.  The second form is for a kernel trace: run it under `rocprofv3 --kernel-trace --stats
-- python scripts/npt_overhead.py --attempts 0` and `... --attempts 20`; the difference of the two kernel counts over 20 is what
one attempt launches.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(nside, barostat_frequency=None, seed=7):
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.openmm import app
    from atomsmm_amd.testing import system_from_arrays, tip3p_box
    case = tip3p_box(nside)
    system = system_from_arrays(case, nonbondedMethod='CutoffPeriodic', cutoff=1.0, switch=0.9)
    respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    outer = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, 1.0 * unit.nanometers, 0.9 * unit.nanometers)
    outer.importFrom(nb)
    outer.setForceGroup(2)
    outer.addTo(respa)
    if barostat_frequency is not None:
        barostat = openmm.MonteCarloBarostat(1.0 * unit.bar, 300.0 * unit.kelvin, barostat_frequency)
        barostat.setRandomNumberSeed(seed)
        respa.addForce(barostat)
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(4.0 * unit.femtoseconds)
    simulation = app.Simulation(app.Topology(len(case['positions'])), respa, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(case['positions'] * unit.nanometers)
    simulation.context.setVelocities(case['velocities'])
    return simulation


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--nside', type=int, default=32)
    ap.add_argument('--frequency', type=int, default=25)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0, help='seconds per timed window, at least')
    ap.add_argument('--attempts', type=int, default=None, help='trace mode: setup, warm-up and this many attempts, nothing timed')
    args = ap.parse_args()
    import torch
    from bench import relax

    if args.attempts is not None:
        simulation = build(args.nside, args.frequency)
        simulation.step(2)
        eng = simulation.context._engine
        for _ in range(args.attempts):
            eng._barostat_attempt()
            simulation.step(1)          # (the forces an accepted move made stale are evaluated again, as in a run)
        torch.cuda.synchronize()
        print(json.dumps(dict(mode='trace', attempts=args.attempts, barostat=eng.barostat_stats, box=eng.ctx.box_stats())))
        return

    plain = build(args.nside)
    relax(plain, torch)
    npt = build(args.nside, args.frequency)
    npt.context.setState(plain.context.getState(getPositions=True, getVelocities=True))
    sims = dict(plain=plain, npt=npt)
    # steps per window: whole attempt intervals, at least `window` seconds of the plain run
    plain.step(2 * args.frequency)
    npt.step(2 * args.frequency)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain.step(2 * args.frequency)
    torch.cuda.synchronize()
    per_step = (time.perf_counter() - t0) / (2 * args.frequency)
    steps = args.frequency * max(2, int(args.window / per_step / args.frequency) + 1)
    eng = npt.context._engine
    stats0, box0 = dict(eng.barostat_stats), eng.ctx.box_stats()
    ms = dict(plain=[], npt=[])
    for _ in range(args.repeats):
        for name in ('plain', 'npt'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sims[name].step(steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    stats1, box1 = eng.barostat_stats, eng.ctx.box_stats()
    attempts = stats1['attempts'] - stats0['attempts']
    best = {name: min(values) for name, values in ms.items()}
    extra_us = (best['npt'] - best['plain']) * args.frequency * 1e3
    print(json.dumps(dict(
        atoms=eng.n, frequency=args.frequency, steps_per_window=steps, ms_per_step=ms, best_ms_per_step=best,
        extra_us_per_attempt=extra_us, extra_steps_per_attempt=extra_us / (best['plain'] * 1e3),
        attempts=attempts, accepted=stats1['accepted'] - stats0['accepted'],
        box_stats_over_windows={k: box1[k] - box0[k] for k in box1}, box_stats_total=box1,
        volume_nm3=float(eng.box.prod()), kernel_revision=__import__('atomsmm_amd.backend', fromlist=['x']).kernel_revision())))


if __name__ == '__main__':
    main()
