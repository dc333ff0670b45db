"""One energy minimisation of the bench's water box (bench.build_simulation: tip3p_box(nside), RESPASystem + DampedSmoothedForce; lattice
start, no relaxation), for a kernel trace of the minimiser's launches next to the force evaluations:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/probe_minimize.py [--nside 32] [--iterations 50]
    python scripts/probe_minimize.py --summarise OUT EVALUATIONS ITERATIONS        # the table kept as profiles/minimize_kernel_stats.txt

Prints one JSON line: iterations, evaluations, energies, wall time."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MINIMISER = ('k_min_gram', 'k_min_coef', 'k_min_combine', 'k_min_trial')


def summarise(directory, evaluations, iterations):
    """Per-iteration time of the four minimiser launches beside the time of one all-group force + energy evaluation: every kernel
    of the trace that is not the minimiser's belongs to an evaluation (or to the few launches of set-up, listed apart)."""
    path = glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True)[0]
    rows = list(csv.DictReader(open(path)))
    mine = {name: next((r for r in rows if name in r['Name']), None) for name in MINIMISER}
    other = [r for r in rows if not any(name in r['Name'] for name in MINIMISER)]
    print('kernel                                                               calls   average us   total us')
    for name, r in mine.items():
        print('%-68s %6s %12.2f %10.1f' % (name, r['Calls'], float(r['AverageNs']) / 1e3, float(r['TotalDurationNs']) / 1e3))
    for r in other[:12]:
        print('%-68s %6s %12.2f %10.1f' % (r['Name'][:68], r['Calls'], float(r['AverageNs']) / 1e3, float(r['TotalDurationNs']) / 1e3))
    per_advance = sum(float(mine[name]['AverageNs']) for name in MINIMISER[:3]) / 1e3
    trial = float(mine['k_min_trial']['AverageNs']) / 1e3
    trials_per_iteration = float(mine['k_min_trial']['Calls']) / max(1, iterations)
    vector = per_advance + trial * trials_per_iteration
    evaluation = sum(float(r['TotalDurationNs']) for r in other) / 1e3 / max(1, evaluations)
    print()
    print('iterations %d, evaluations %d, trials per iteration %.2f' % (iterations, evaluations, trials_per_iteration))
    print('minimiser launches per iteration (Gram update + coefficients + combination + trials): %.1f us' % vector)
    print('one all-group force + energy evaluation (all other kernels / evaluations):          %.1f us' % evaluation)
    print('ratio: %.3f' % (vector / evaluation))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nside', type=int, default=32)
    ap.add_argument('--iterations', type=int, default=50)
    ap.add_argument('--summarise', nargs=3, metavar=('DIR', 'EVALUATIONS', 'ITERATIONS'))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise[0], int(args.summarise[1]), int(args.summarise[2]))
    import torch
    import bench
    simulation, _case = bench.build_simulation(args.nside, (4, 2, 1), 4.0)
    context = simulation.context
    e0 = context.getState(getEnergy=True).getPotentialEnergy()._value
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = context._engine.minimize(10.0, args.iterations, None)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    e1 = context.getState(getEnergy=True).getPotentialEnergy()._value
    print(json.dumps(dict(atoms=context._engine.n, iterations=info['iterations'], evaluations=info['evaluations'], reason=info['reason'],
                          energy_start=e0, energy_end=e1, seconds=round(seconds, 4),
                          ms_per_evaluation=round(1e3 * seconds / info['evaluations'], 4))), flush=True)


if __name__ == '__main__':
    main()
