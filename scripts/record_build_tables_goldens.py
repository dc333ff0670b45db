#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_build_tables.py: the molecule-row list build (csrc/cluster.hip: k_cbuild) loads a cell's stencil
tables, made once per rebuild by the sort launch, instead of making them in every wavefront, and drains a row's short leftover one
survivor per lane.  Neither may change an entry of a row or its place: the forces keep their bits.

    python scripts/record_build_tables_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/build_tables_<case>.npz (or DIR/...): for every evaluation of the case the group-1 (near) and group-2 (outer)
forces -- fp64, of a seeded choice of 512 atoms of a box with more than 1 536 atoms (golden_atoms of
scripts/record_pair_prologue_goldens.py) together with the SHA-256 of the whole array, so that every atom is pinned -- and the list's
entry counts (pair_stats: n_list_pairs of the outer force = 9 x entries, of the near force = 9 x front entries).  The files in the
repository were recorded by the build of the commit BEFORE the tables moved (kernel revision r07-triploop); the test asks for the
same bits.  Cases with `world` run that many ranks as threads of one process (engine.LocalWorld): every rank's forces and its own
slice's counts are kept."""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
_spec = importlib.util.spec_from_file_location('record_pair_prologue_goldens', os.path.join(ROOT, 'scripts', 'record_pair_prologue_goldens.py'))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

RC_OUTER = 1.0          # nm: cutoff of the outer force = the list owner's; list radius = RC_OUTER + Skin
# name -> waters per box edge, Verlet buffer (None: the library's default, 0.1 nm), ranks, whether a second build follows
#   box8               1 536 atoms, 3 cells per edge: the per-pair-image build, a stencil that wraps onto itself
#   box17              14 739 atoms, 7 cells per edge: shift codes, interior and edge cells; then every molecule is moved by more than
#                      the buffer (`moved`) and the forces are taken again: a second build whose tables must be its own
#   box12_leftover_1   5 184 atoms, 5 cells per edge, Skin 0.06: every row's sphere holds 257 first atoms: a leftover of ONE survivor
#   box12_leftover_123 Skin 0.04: 251 first atoms, a leftover of 123 (the packed two-halves drain)
#   box8_two_ranks, box12_two_ranks: a rank's slice of the rows (per-pair image / shift codes)
CASES = {
    'box8': dict(nside=8, skin=None, world=1, moved=False),
    'box17': dict(nside=17, skin=None, world=1, moved=True),
    'box12_leftover_1': dict(nside=12, skin=0.06, world=1, moved=False),
    'box12_leftover_123': dict(nside=12, skin=0.04, world=1, moved=False),
    'box8_two_ranks': dict(nside=8, skin=0.1, world=2, moved=False),
    'box12_two_ranks': dict(nside=12, skin=0.1, world=2, moved=False),
}


def displaced(c):
    """Every molecule moved as a whole along a smooth field of amplitude 0.12 nm (more than any Verlet buffer here; neighbours move
    less than 0.05 nm against each other: no close contacts), which also takes the box off its lattice."""
    x, L = c['positions'], c['box']
    x0 = np.repeat(x[0::3], 3, axis=0)
    ph = 2.0 * np.pi * x0 / L
    d = 0.12 * np.stack([np.sin(ph[:, 1]) * np.cos(ph[:, 2]), np.sin(ph[:, 2] + 1.0), np.cos(ph[:, 0] + 2.0) * np.sin(ph[:, 1] + 0.5)], axis=1)
    return x + d


def sphere_counts(c, skin):
    """Candidates that pass the build's sphere test, per row molecule (the molecule itself included): first atoms closer than list
    radius + both extents.  A row's ring is drained whenever it holds 128: the last drain takes count mod 128."""
    x, L = c['positions'], c['box']
    x0 = x[0::3]
    ext = np.maximum(np.linalg.norm(x[1::3] - x0, axis=1), np.linalg.norm(x[2::3] - x0, axis=1)) * 1.000001 + 1e-6
    out = np.empty(len(x0), dtype=np.int64)
    for a in range(0, len(x0), 512):
        d = x0[a:a + 512, None, :] - x0[None, :, :]
        d -= L * np.round(d / L)
        out[a:a + 512] = (np.sqrt((d * d).sum(-1)) < RC_OUTER + skin + ext[a:a + 512, None] + ext[None, :]).sum(1)
    return out


def _run(case, c):
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.openmm import app
    from atomsmm_amd.testing import system_from_arrays
    system = system_from_arrays(c, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    f = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, RC_OUTER * unit.nanometers, 0.9 * unit.nanometers).importFrom(nb)
    f.setForceGroup(2)
    f.addTo(respa)
    integrator = atomsmm.RespaPropagator([4, 2, 1]).integrator(4.0 * unit.femtoseconds)
    props = {} if case['skin'] is None else {'Skin': repr(case['skin'])}
    sim = app.Simulation(app.Topology(), respa, integrator, openmm.Platform.getPlatformByName('HIP'), props)
    context = sim.context
    eng = context._engine
    context.setPositions(c['positions'] * unit.nanometers)
    context.setVelocities(c['velocities'])
    near, outer = eng.pair_force_ids(1)[0], eng.pair_force_ids(2)[0]

    def stats(tag, out):
        sn, so = eng.ctx.pair_stats(near), eng.ctx.pair_stats(outer)
        assert sn['list_kind'] == 1 and so['list_kind'] == 1, 'molecule rows expected'
        out['pairs_near' + tag] = np.int64(sn['n_list_pairs'])
        out['pairs_outer' + tag] = np.int64(so['n_list_pairs'])
        out['builds' + tag] = np.int64(so['n_builds'])
        out['rlist'] = np.float64(so['rlist'])
        out['slice_atoms'] = np.int64(so['n_slice_atoms'])
        out['n_cells'] = np.int64(so['n_cells'])
    out = {}
    out['f1'], out['f2'] = P.group_forces(context)
    stats('', out)
    if case['moved']:
        context.setPositions(displaced(c) * unit.nanometers)
        out['f1_moved'], out['f2_moved'] = P.group_forces(context)
        stats('_moved', out)
    eng.ctx.check()
    eng.ctx.close()
    return out


def run_case(case):
    """-> (system arrays, [dict of results per rank])."""
    from atomsmm_amd.testing import tip3p_box
    c = tip3p_box(case['nside'])
    if case['world'] == 1:
        return c, [_run(case, c)]
    from atomsmm_amd.engine import LocalWorld
    return c, LocalWorld(case['world']).run(lambda rank: _run(case, c))


FORCES = ('f1', 'f2', 'f1_moved', 'f2_moved')


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def condensed(results):
    """What a golden keeps of run_case's results: rank r's entries under 'r<r>_...'."""
    keep = {}
    for r, out in enumerate(results):
        rows = P.golden_atoms(len(out['f1']))
        for k, v in out.items():
            if k in FORCES:
                keep['r%d_%s' % (r, k)] = np.asarray(v, dtype=np.float64)[rows]
                keep['r%d_%s_sha256' % (r, k)] = np.array(digest(v))
            elif k.startswith('pairs_'):
                keep['r%d_%s' % (r, k)] = v
    return keep


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'build_tables_%s.npz' % name)


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
        c, results = run_case(CASES[name])
        path = golden_path(name, where)
        np.savez_compressed(path, **condensed(results))
        for r, out in enumerate(results):
            print(name, 'rank', r, {k: (np.shape(v) if k in FORCES else v.item()) for k, v in out.items()}, flush=True)
            assert all(np.all(np.isfinite(out[k])) for k in FORCES if k in out)
        print(name, '%.0f KB' % (os.path.getsize(path) / 1024.0), flush=True)
