"""Cost of regulated dynamics on the C3 box (98 304 atoms, DampedSmoothedForce outer, RESPA [4,2,1] at 4 fs): NHL_R against the
regulated massive Nose-Hoover-Langevin composition (RegulatedTranslation / RegulatedBoost / RegulatedMassiveNHL in the middle of
the innermost loop) run as native ops, and the same with native recognition off (per-DOF expressions):

    python scripts/probe_regulated.py [--steps K] [names...]          names: NHL_R, regulated, regulated_general

Kernels per step come from a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/probe_regulated.py --steps K
NAME` (launches divided by the steps of that run, warm-up included).  Results: profiles/regulated_c3.txt."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import engine, openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.testing import system_from_arrays, tip3p_box  # noqa: E402

fs, K, ps = unit.femtoseconds, unit.kelvin, unit.picoseconds


def regulated():
    return atomsmm.MultipleTimeScaleIntegrator(4 * fs, [4, 2, 1], move=atomsmm.RegulatedTranslationPropagator(300 * K, 2),
                                               boost=atomsmm.RegulatedBoostPropagator(),
                                               bath=atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(300 * K, 2, 10 * fs, 1 / ps))


MAKE = {'NHL_R': (lambda: atomsmm.NHL_R_Integrator(4 * fs, [4, 2, 1], 300 * K, 10 * fs, 1 / ps), True),
        'regulated': (regulated, True), 'regulated_general': (regulated, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('names', nargs='*')
    args = ap.parse_args()
    case = tip3p_box(32)
    for name in args.names or list(MAKE):
        make, native = MAKE[name]
        engine.Engine.native_regulated = native
        system = system_from_arrays(case, nonbondedMethod='CutoffPeriodic', cutoff=1.0, switch=0.9)
        respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
        nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
        outer = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, 1.0 * unit.nanometers, 0.9 * unit.nanometers).importFrom(nb)
        outer.setForceGroup(2)
        outer.addTo(respa)
        integ = make()
        integ.setRandomNumberSeed(5)
        sim = app.Simulation(app.Topology(len(case['positions'])), respa, integ, openmm.Platform.getPlatformByName('HIP'))
        sim.context.setPositions(case['positions'] * unit.nanometers)
        sim.context.setVelocities(case['velocities'])
        sim.step(args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.step(args.steps)
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / args.steps
        eng = sim.context._engine
        # (EXPR ops of the steady-state program: the first step's program differs only in its force evaluations)
        exprs = max(sum(op.op == 6 for op in prog[0]) for prog in eng._programs.values()) if not eng._interpreted else -1
        print('%-18s ms/step %.3f  ns/day %6.1f  interpreted = %s  EXPR ops/step = %d  steps = %d + %d' % (
            name, t * 1e3, 4e-6 * 86400 / t, eng._interpreted, exprs, args.warmup, args.steps), flush=True)
        del sim


if __name__ == '__main__':
    main()
