#!/usr/bin/env python3
"""What a step of LangevinMiddleIntegrator(300 K, 1/ps, 2 fs) on rigid water costs, three ways:

    native   the engine's step for a stock integrator: EVAL ; STOCK (one launch for the whole post-force update, csrc/stock.hip)
    off      the same with Engine.set_stock_native(False): the step from KICK, CONSTRAIN_V, MOVE, BATH, MOVE, COPY, CONSTRAIN_X, EXPR
    custom   the CustomIntegrator program of OpenMM's documentation for this scheme (`v+dt*f/m` ... `v+(x-x1)/dt`) -- how the
             protocol had to be written before the stock classes existed; this variant also runs on a checkout without them

on q-SPC-FW (1 536 atoms, tests/golden) or on a synthetic rigid TIP3P box (`--nside 32`: 98 304 atoms).  Reports the ops scheduled per step
(amm_run_stats: scheduling decisions, one per op or fused run of ops -- an evaluation counts as one whatever it launches) and milliseconds per step from device events.

    python scripts/stock_step.py [--system spcfw|box] [--nside 32] [--variants native,off,custom] [--steps 200] [--repeats 5]

All variants live in one process, start from the same relaxed state and are timed in turn (alternating, `--repeats` windows of
`--steps` steps each after a warm-up window): the spread of a variant's windows is what a difference between two variants has to
exceed.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPERATURE, FRICTION, DT_FS = 300.0, 1.0, 2.0


def case_of(args):
    import numpy as np
    if args.system == 'spcfw':
        data = np.load(os.path.join(ROOT, 'tests', 'golden', 'q-SPC-FW.npz'))
        case = {k: data[k] for k in data.files}
        kT = 0.0083144626181532 * TEMPERATURE
        case['velocities'] = np.random.default_rng(1).normal(size=case['positions'].shape) * np.sqrt(kT / case['mass'])[:, None]
        return case
    from atomsmm_amd.testing import tip3p_box
    case = tip3p_box(args.nside)
    case['residue'] = np.repeat(np.arange(len(case['mass']) // 3), 3)
    return case


def integrator_of(variant):
    import math
    from atomsmm_amd import openmm, unit
    if variant != 'custom':
        return openmm.LangevinMiddleIntegrator(TEMPERATURE * unit.kelvin, FRICTION / unit.picosecond, DT_FS * unit.femtoseconds)
    dt = DT_FS * 1e-3
    integrator = openmm.CustomIntegrator(dt)
    integrator.addGlobalVariable('a', math.exp(-FRICTION * dt))
    integrator.addGlobalVariable('b', math.sqrt(1.0 - math.exp(-2.0 * FRICTION * dt)))
    integrator.addGlobalVariable('kT', unit.BOLTZMANN_CONSTANT_kB._value * TEMPERATURE)
    integrator.addPerDofVariable('x1', 0)
    integrator.addUpdateContextState()
    integrator.addComputePerDof('v', 'v + dt*f/m')
    integrator.addConstrainVelocities()
    integrator.addComputePerDof('x', 'x + 0.5*dt*v')
    integrator.addComputePerDof('v', 'a*v + b*sqrt(kT/m)*gaussian')
    integrator.addComputePerDof('x', 'x + 0.5*dt*v')
    integrator.addComputePerDof('x1', 'x')
    integrator.addConstrainPositions()
    integrator.addComputePerDof('v', 'v + (x-x1)/dt')
    return integrator


def build(case, variant):
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.openmm import app
    from atomsmm_amd.testing import system_from_arrays
    system = system_from_arrays(case, nonbondedMethod='CutoffPeriodic', rigidWater=True)
    nb = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb).addTo(system)
    integrator = integrator_of(variant)
    integrator.setRandomNumberSeed(11)
    simulation = app.Simulation(app.Topology(len(case['positions'])), system, integrator, openmm.Platform.getPlatformByName('HIP'))
    if variant == 'off':
        simulation.context._engine.set_stock_native(False)
    simulation.context.setPositions(case['positions'] * unit.nanometers)
    simulation.context.applyConstraints()
    simulation.context.setVelocities(case['velocities'])
    simulation.context.applyVelocityConstraints()
    return simulation


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--system', choices=['spcfw', 'box'], default='spcfw')
    ap.add_argument('--nside', type=int, default=32)
    ap.add_argument('--variants', default='native,off,custom')
    ap.add_argument('--steps', type=int, default=200, help='steps per timed window')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--relax', type=int, default=None, help='steps of velocity-rescaling relaxation of the lattice start (box: 600)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stock_step.py measures on the GPU: none found')
    variants = args.variants.split(',')
    case = case_of(args)
    sims = {}
    for variant in variants:
        sims[variant] = build(case, variant)
    first = sims[variants[0]]
    relax_steps = args.relax if args.relax is not None else (600 if args.system == 'box' else 0)
    if relax_steps:
        from bench import relax
        relax(first, torch, max_steps=relax_steps)
    state = first.context.getState(getPositions=True, getVelocities=True)
    for variant in variants[1:]:
        sims[variant].context.setState(state)
    scheduled, windows = {}, {v: [] for v in variants}
    for variant in variants:                       # warm-up: every program compiled, every list built
        sims[variant].step(args.steps)
        ctx = sims[variant].context._engine.ctx
        stats = ctx.run_stats() if hasattr(ctx, 'run_stats') else {}
        if 'scheduled' in stats:
            sims[variant].step(20)
            scheduled[variant] = (ctx.run_stats()['scheduled'] - stats['scheduled']) / 20.0
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for variant in variants:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            sims[variant].step(args.steps)
            stop.record()
            stop.synchronize()
            windows[variant].append(start.elapsed_time(stop) / args.steps)
    out = dict(system=args.system, atoms=len(case['positions']), steps_per_window=args.steps, ops_scheduled_per_step=scheduled, ms_per_step={})
    for variant in variants:
        w = sorted(windows[variant])
        out['ms_per_step'][variant] = dict(median=w[len(w) // 2], min=w[0], max=w[-1], windows=windows[variant])
        sims[variant].context._engine._check()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
