"""Cost of one report of the potential energy at K lambda_vdw states at config C5 (bench.build_simulation_c5: ~249 000 atoms, AFED on
lambda_vdw): the reference reporters' way (setParameter + getState(getEnergy=True) per state, then restore) against
Engine.energies_at_states (one evaluation of the lambda-independent forces + one amm_pair_energy_states launch), and the time of the
step() that follows each (the reference's way leaves stale forces and cleared step programs behind it).

    python scripts/probe_state_energies.py [--states 11 21] [--repeat 5] [--new-only]

Prints one JSON line per K (milliseconds, medians over --repeat reports).  --new-only: the new path alone (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--states', type=int, nargs='+', default=[11, 21, 64])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--new-only', action='store_true')
    args = ap.parse_args()
    import torch
    import bench
    simulation, _case = bench.build_simulation_c5((4, 2, 1), 2.0)
    context = simulation.context
    eng = context._engine
    simulation.step(4)                                     # lists built, programs compiled

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        return value, 1e3 * (time.perf_counter() - t0)

    def reference_report(lam):
        here = context.getParameter('lambda_vdw')
        out = []
        for value in lam:
            context.setParameter('lambda_vdw', float(value))
            out.append(context.getState(getEnergy=True).getPotentialEnergy()._value)
        context.setParameter('lambda_vdw', here)
        return np.array(out)

    _, plain_step = timed(lambda: simulation.step(1))
    # one getState(getEnergy=True) right after a step: what ONE state of the reference loop costs there (the first evaluation after a
    # step re-checks the lists and gathers the sorted copies; the later states of the loop find them current)
    after_step = []
    for _ in range(args.repeat):
        simulation.step(1)
        after_step.append(timed(lambda: context.getState(getEnergy=True))[1])
    soft = [e.softcore['pid'] for e in eng.entries if e.softcore is not None][0]
    for K in args.states:
        lam = np.linspace(0.0, 1.0, K)
        rows = {'new': [], 'new_next_step': [], 'ref': [], 'ref_next_step': []}
        diff = 0.0
        walks = []
        for _ in range(args.repeat):
            w0 = eng.ctx.pair_stats(soft)['n_candidate_walks']
            got, t = timed(lambda: eng.energies_at_states(['lambda_vdw'], lam[:, None]))
            walks.append(eng.ctx.pair_stats(soft)['n_candidate_walks'] - w0)
            rows['new'].append(t)
            rows['new_next_step'].append(timed(lambda: simulation.step(1))[1])
            if args.new_only:
                continue
            got = eng.energies_at_states(['lambda_vdw'], lam[:, None])
            ref, t = timed(lambda: reference_report(lam))          # (same positions as `got`)
            rows['ref'].append(t)
            rows['ref_next_step'].append(timed(lambda: simulation.step(1))[1])
            diff = max(diff, float(np.abs(got - ref).max() / np.abs(ref).max()))
        line = {'config': 'C5', 'K': K, 'ms_plain_step': round(plain_step, 3),
                'ms_one_getstate_energy_after_step': round(float(np.median(after_step)), 3), 'states_launches_on_candidates': walks}
        for key, values in rows.items():
            if values:
                line['ms_' + key] = round(float(np.median(values)), 3)
        line['max_rel_diff_vs_reference_loop'] = diff
        line['fallbacks'] = eng.n_state_fallbacks
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
