"""Record the 50-digit checker's answers for the large GayBerneForce cases (tests/gayberne_cases.py: RECORDED) into
tests/golden/data/gayberne_<name>.npz: the settled positions, the energy, the forces by central differences, the closest contact
ratio, the largest rho and the number of interacting pairs.  Pure CPU; the force rows are dealt to worker processes.

    python scripts/record_gayberne_goldens.py [--jobs N] [name ...]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import gayberne_cases as GC  # noqa: E402

_CASE = {}


def _rows(job):
    name, rows = job
    spec, pos = _CASE[name]
    out = GC.evaluate(spec, pos, rows=rows)
    return rows, out['forces'][rows], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument('names', nargs='*', default=sorted(GC.RECORDED))
    args = ap.parse_args()
    jobs = []
    for name in args.names:
        spec, pos, _ = GC.RECORDED[name]()
        _CASE[name] = (spec, pos)
        order = list(range(len(pos)))
        per = max(1, -(-len(order) // (4 * args.jobs)))
        jobs += [(name, order[k:k + per]) for k in range(0, len(order), per)]
    forces = {name: np.full((len(_CASE[name][1]), 3), np.nan) for name in args.names}
    scalars = {}
    with multiprocessing.get_context('fork').Pool(args.jobs) as pool:       # (fork: the workers inherit _CASE)
        for (name, _), (rows, f, out) in zip(jobs, pool.imap(_rows, jobs)):
            forces[name][rows] = f
            scalars[name] = out
    os.makedirs(GC.GOLDEN, exist_ok=True)
    for name in args.names:
        out = scalars[name]
        assert np.isfinite(forces[name]).all()
        np.savez(GC.golden_path(name), positions=_CASE[name][1], energy=out['energy'], forces=forces[name], min_ratio=out['min_ratio'],
                 max_rho=out['max_rho'], n_pairs=out['n_pairs'])
        print('%s: %d particles, %d pairs, E = %.15g, closest contact %.4f, largest rho %.4f' %
              (name, len(forces[name]), out['n_pairs'], out['energy'], out['min_ratio'], out['max_rho']), flush=True)


if __name__ == '__main__':
    main()
