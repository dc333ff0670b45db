#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_pair_prologue.py: what the molecule-row pair kernels compute must not depend on how they
stage their tables or fetch a task's rows.

    python scripts/record_pair_prologue_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/pair_prologue_<case>.npz (or DIR/..., fp64): the group-1 and group-2 forces of one evaluation and positions and
velocities after 6 outer steps of RESPA [4, 2, 1] -- of every atom for the 1 536-atom boxes, of a seeded choice of 512 atoms
(golden_atoms) for the larger ones.  The files in the repository were recorded by the build of the commit BEFORE the kernels got
their table image and row prologue (kernel revision r05-epi5); the test asks for the same bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# name -> box side (molecules per edge), RESPASystem(rc, rs) in nm, library options, whether the charges are rescaled in between
CASES = {
    'box8': dict(nside=8, rc=0.7, rs=0.5, options=()),                             # per-pair minimum image; most wavefronts idle
    'box11': dict(nside=11, rc=0.7, rs=0.5, options=()),                           # 1 331 rows: several phases, a ragged last task
    'box12_one_phase': dict(nside=12, rc=0.7, rs=0.5, options=(('row_phases', 0),)),
    'box12_lanes8': dict(nside=12, rc=0.7, rs=0.5, options=(('lanes_per_row', 8),)),
    'box8_other_tables': dict(nside=8, rc=0.6, rs=0.45, options=()),               # other table sizes: another remainder of the copy
    'box8_set_params': dict(nside=8, rc=0.6, rs=0.45, options=(('positions_private', 1),), rescale=0.9),
    'box14_two_tasks': dict(nside=14, rc=0.7, rs=0.5, options=(('lanes_per_row', 64),)),   # 2 744 one-row tasks: more than wavefronts
    # 4 913 rows at 32 lanes each: a round of two-row tasks for every wavefront, the remainder as one-row tasks -- two phases
    'box17_two_phases': dict(nside=17, rc=0.7, rs=0.5, options=(('lanes_per_row', 32),)),
}
STEPS = 6
SUBSET = 512


def golden_atoms(n):
    """The atoms a golden keeps: all of a small box, a seeded choice of SUBSET of a larger one (sorted)."""
    if n <= 1536:
        return np.arange(n)
    return np.sort(np.random.default_rng(20261017).choice(n, SUBSET, replace=False))


def build_context(case):
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.testing import system_from_arrays, tip3p_box
    c = tip3p_box(case['nside'])
    system = system_from_arrays(c, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, case['rc'] * unit.nanometers, case['rs'] * unit.nanometers)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    f = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, 1.0 * unit.nanometers, 0.9 * unit.nanometers).importFrom(nb)
    f.setForceGroup(2)
    f.addTo(respa)
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(4.0 * unit.femtoseconds)
    context = openmm.Context(respa, integrator, openmm.Platform.getPlatformByName('HIP'))
    for name, value in case['options']:
        context._engine.ctx.set_option(name, value)
    context.setPositions(c['positions'] * unit.nanometers)
    context.setVelocities(c['velocities'])
    return c, context, integrator


def group_forces(context):
    return [context.getState(getForces=True, groups={g}).getForces(asNumpy=True)._value.copy() for g in (1, 2)]


def run_case(case):
    """-> (system arrays, dict of results).  f1, f2: one evaluation; f1_rescaled, f2_rescaled: again at the same positions after
    amm_pair_set_params scaled every charge (cases with `rescale`); x, v: after STEPS outer steps."""
    c, context, integrator = build_context(case)
    eng = context._engine
    out = {}
    out['f1'], out['f2'] = group_forces(context)
    if case.get('rescale'):
        for group in (1, 2):
            for pid in eng.pair_force_ids(group):
                eng.ctx.pair_set_params(pid, case['rescale'] * c['charge'], c['sigma'], c['epsilon'])
        out['f1_rescaled'], out['f2_rescaled'] = group_forces(context)
        for group in (1, 2):
            for pid in eng.pair_force_ids(group):
                eng.ctx.pair_set_params(pid, c['charge'], c['sigma'], c['epsilon'])
    integrator.step(STEPS)
    st = context.getState(getPositions=True, getVelocities=True)
    out['x'] = st.getPositions(asNumpy=True)._value.copy()
    out['v'] = st.getVelocities(asNumpy=True)._value.copy()
    out['list_kind'] = np.int64(eng.ctx.pair_stats(eng.pair_force_ids(1)[0])['list_kind'])
    eng.ctx.check()
    return c, out


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'pair_prologue_%s.npz' % name)


if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'          # (before the library is loaded: torch brings its own HIP runtime)
    from atomsmm_amd import backend
    print('kernel revision', backend.kernel_revision())
    args = sys.argv[1:]
    where = GOLDEN
    if args and args[0] == '--out':
        where = args[1]
        args = args[2:]
        os.makedirs(where, exist_ok=True)
    for name in (args or sorted(CASES)):
        _, out = run_case(CASES[name])
        assert out['list_kind'] == 1, 'molecule rows expected'
        path = golden_path(name, where)
        keep = golden_atoms(len(out['x']))
        np.savez_compressed(path, **{k: np.asarray(v, dtype=np.float64)[keep] for k, v in out.items() if k != 'list_kind'})
        print(name, {k: np.shape(v) for k, v in out.items()}, '%.0f KB' % (os.path.getsize(path) / 1024.0), flush=True)
