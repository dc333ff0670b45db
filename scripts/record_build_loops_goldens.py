#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_build_loops.py: the molecule-row list build (csrc/cluster.hip: k_cbuild) keeps a row's sphere
constants and ring state in scalar registers over the candidate stream, tests the rows of a batch in unrolled code and drains the rows
whose ring is full from a scalar pending mask.  None of it may change an entry of a row or its place: the forces keep their bits.

    python scripts/record_build_loops_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard
    python scripts/record_build_loops_goldens.py --events [case ...]        # no GPU: which paths of the build a case reaches

writes tests/golden/build_loops_<case>.npz (or DIR/...): for every evaluation of the case the group-1 (near) and group-2 (outer)
forces -- fp64, of a seeded choice of 512 atoms of a box with more than 1 536 atoms (golden_atoms of
scripts/record_pair_prologue_goldens.py) together with the SHA-256 of the whole array, so that every atom is pinned -- and the list's
entry counts (pair_stats: n_list_pairs of the outer force = 9 x entries, of the near force = 9 x front entries).  The files in the
repository were recorded by the build of the commit BEFORE the loops changed (kernel revision r10-lookupoffset); the test asks for the
same bits.  Cases with `world` run that many ranks as threads of one process (engine.LocalWorld): every rank's forces and its own
slice's counts are kept.

Which paths a case reaches is worked out on the CPU (stream_events: the build's cells, parts, batches, candidate stream and sphere test
in numpy) and printed with every recording: sizes of the batches (rows that the unrolled test skips), chunk pairs of a cell's stream,
what a row leaves for the final drain (<= 64: one survivor per lane; more: two), and how many rows of one batch filled their ring in
the same chunk pair (the pending mask)."""
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
DEFAULT_SKIN = 0.1      # nm: the library's Verlet buffer
BATCH = 5               # row molecules of a batch (CB_BATCH of csrc/cluster.hip)
# name -> waters per box edge, number density (None: water, 33.368 / nm^3), Verlet buffer (None: the library's default), ranks,
# `then`: what follows the first evaluation (None; 'moved': every molecule beyond the buffer, a second build; 'squeezed': the middle
# of the box contracted until rows outgrow the capacity that the first build chose), `shaken`: start from the moved positions
#   box8               1 536 atoms, 3 cells per edge: images per atom pair (RINT), a stencil that wraps; 4 chunk pairs
#   box5_sparse        375 atoms in 2.5 nm: the whole box is ONE chunk pair of 125 candidates (RINT)
#   box7_sparse        1 029 atoms in 2.58 nm: 343 candidates = 3 chunk pairs, the last of 87 (RINT)
#   box12              5 184 atoms, 5 cells per edge, cells of 8, 12, 18 and 27 molecules in 5 parts: batches of 2, 3, 4, 5 and 1 rows
#   box17              14 739 atoms, 7 cells per edge: shift codes, streams of 14, 15, 16 and 18 chunk pairs (14 and 15 after the move); then a second build
#   box12_shaken_*     5 184 atoms off the lattice at two Verlet buffers: rows of many lengths.  0.05 nm: 247 to 270 survivors, leftovers
#                      of 119 .. 127 and 0 .. 14 (1 and 127 among them); 0.12 nm: 305 to 329, leftovers of 49 .. 73 (64 and 65 among them)
#   box12_squeezed     rows overflow in the second build
#   box8_two_ranks, box12_two_ranks: a rank's slice of the rows (the SLICE instantiations)
CASES = {
    'box8': dict(nside=8),
    'box5_sparse': dict(nside=5, density=8.0),
    'box7_sparse': dict(nside=7, density=20.0),
    'box12': dict(nside=12),
    'box17': dict(nside=17, then='moved'),
    'box12_shaken_s05': dict(nside=12, skin=0.05, shaken=True),
    'box12_shaken_s12': dict(nside=12, skin=0.12, shaken=True),
    'box12_squeezed': dict(nside=12, then='squeezed'),
    'box8_two_ranks': dict(nside=8, skin=0.1, world=2),
    'box12_two_ranks': dict(nside=12, skin=0.1, world=2),
}
for _case in CASES.values():
    for _k, _v in dict(density=None, skin=None, world=1, then=None, shaken=False).items():
        _case.setdefault(_k, _v)


def displaced(c, x=None):
    """Every molecule moved as a whole along a smooth field of amplitude 0.12 nm (more than any Verlet buffer here; neighbours move
    less than 0.05 nm against each other: no close contacts), which also takes the box off its lattice."""
    x, L = c['positions'] if x is None else x, c['box']
    x0 = np.repeat(x[0::3], 3, axis=0)
    ph = 2.0 * np.pi * x0 / L
    d = 0.12 * np.stack([np.sin(ph[:, 1]) * np.cos(ph[:, 2]), np.sin(ph[:, 2] + 1.0), np.cos(ph[:, 0] + 2.0) * np.sin(ph[:, 1] + 0.5)], axis=1)
    return x + d


def squeezed(c, radius=1.5, factor=0.72):
    """The molecules whose first atom lies within `radius` of the box centre moved, each as a whole, towards it: distances shrink by
    `factor`, the density there grows by 1 / factor^3 = 2.7 -- more than the 1.5 x + 32 entries of room that the first build gave a row."""
    x, L = c['positions'], c['box']
    x0 = x[0::3]
    d = x0 - 0.5 * L
    inside = np.linalg.norm(d, axis=1) < radius
    move = np.where(inside[:, None], (factor - 1.0) * d, 0.0)
    return x + np.repeat(move, 3, axis=0)


def start_positions(case, c):
    return displaced(c) if case['shaken'] else c['positions']


def second_positions(case, c):
    return {'moved': displaced, 'squeezed': squeezed}[case['then']](c)


def stream_events(x, L, rlist, parts=None):
    """The list build of a whole box (one rank) on the CPU, as far as its control flow goes: cells of half a reach, `parts` wavefronts
    per cell, batches of BATCH rows, the stencil's molecules as one stream in chunk pairs of 128, a ring per row that is drained at 128.
    -> dict(n_cells, parts, batch_sizes, chunk_pairs, leftovers (what the final drain of a row takes; 0: none), max_pending (rows of
    one batch that reach 128 in the same chunk pair), full_drains, survivors (min, max per row))."""
    x0 = x[0::3]
    nmol = len(x0)
    e = np.maximum(np.linalg.norm(x[1::3] - x0, axis=1), np.linalg.norm(x[2::3] - x0, axis=1))
    ext = e * 1.000001 + 1e-6
    rext = max(1.5 * e.max(), e.max() + 0.05)
    reach = rlist + 2.0 * rext
    nc = np.clip(np.floor(L / (0.5 * reach)).astype(int), 1, 512)
    ncell = int(nc.prod())
    w = x0 - L * np.floor(x0 / L)
    ck = np.minimum((w * nc / L).astype(int), nc - 1)
    cell = (ck[:, 2] * nc[1] + ck[:, 1]) * nc[0] + ck[:, 0]
    order = np.argsort(cell, kind='stable')          # sorted slots: by cell, then by molecule index
    start = np.searchsorted(cell[order], np.arange(ncell + 1))
    if parts is None:
        parts = max(1, min(16, int(np.ceil(1.5 * nmol / ncell / BATCH))))
    ns = np.where(nc >= 5, 5, nc)
    ev = dict(n_cells=ncell, parts=parts, batch_sizes=set(), chunk_pairs=set(), leftovers=set(), max_pending=0, full_drains=0,
              survivors=(10 ** 9, 0))
    for c in range(ncell):
        rows = order[start[c]:start[c + 1]]
        if len(rows) == 0:
            continue
        cx, cy, cz = c % nc[0], (c // nc[0]) % nc[1], c // (nc[0] * nc[1])
        pieces = []
        for oz in range(ns[2]):
            for oy in range(ns[1]):
                for ox in range(ns[0]):
                    nx = ox if nc[0] < 5 else (cx - 2 + ox) % nc[0]
                    ny = oy if nc[1] < 5 else (cy - 2 + oy) % nc[1]
                    nz = oz if nc[2] < 5 else (cz - 2 + oz) % nc[2]
                    cc = (nz * nc[1] + ny) * nc[0] + nx
                    pieces.append(order[start[cc]:start[cc + 1]])
        stream = np.concatenate(pieces)
        npairs = (len(stream) + 127) // 128
        ev['chunk_pairs'].add(npairs)
        d = x0[rows][:, None, :] - x0[stream][None, :, :]
        d -= L * np.round(d / L)
        hit = (d * d).sum(-1) < (rlist + ext[rows][:, None] + ext[stream][None, :]) ** 2
        hit = np.concatenate([hit, np.zeros((len(rows), npairs * 128 - len(stream)), dtype=bool)], axis=1)
        per_pair = hit.reshape(len(rows), npairs, 128).sum(-1)
        tot = per_pair.sum(1)
        ev['survivors'] = (min(ev['survivors'][0], int(tot.min())), max(ev['survivors'][1], int(tot.max())))
        per = (len(rows) + parts - 1) // parts
        for part in range(parts):
            a_end = min((part + 1) * per, len(rows))
            for tb in range(part * per, a_end, BATCH):
                nt = min(BATCH, a_end - tb)
                ev['batch_sizes'].add(nt)
                q = np.zeros(nt, dtype=int)
                for k in range(npairs):
                    q += per_pair[tb:tb + nt, k]
                    pend = q >= 128
                    ev['max_pending'] = max(ev['max_pending'], int(pend.sum()))
                    ev['full_drains'] += int(pend.sum())
                    q[pend] -= 128
                ev['leftovers'].update(int(v) for v in q)
    return ev


def case_events(case, second=False):
    from atomsmm_amd.testing import tip3p_box
    c = tip3p_box(case['nside']) if case['density'] is None else tip3p_box(case['nside'], density=case['density'])
    x = second_positions(case, c) if second else start_positions(case, c)
    return stream_events(x, c['box'], RC_OUTER + (DEFAULT_SKIN if case['skin'] is None else case['skin']))


def _run(case, c):
    import atomsmm_amd as atomsmm
    from atomsmm_amd import backend, openmm, unit
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
    context.setPositions(start_positions(case, c) * unit.nanometers)
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
    eng.ctx.check()
    if case['then']:
        tag = '_' + case['then']
        context.setPositions(second_positions(case, c) * unit.nanometers)
        # (rows that outgrow their capacity: the build raises the overflow flag and leaves those rows EMPTY -- the forces are those of
        # the other rows -- and the check reports it; whichever call reports it, its message is kept)
        out['error' + tag] = ''
        try:
            out['f1' + tag], out['f2' + tag] = P.group_forces(context)
        except backend.HipError as exc:
            out['error' + tag] = str(exc)
        stats(tag, out)
        try:
            eng.ctx.check()
        except backend.HipError as exc:
            out['error' + tag] = out['error' + tag] or str(exc)
    eng.ctx.close()
    return out


def run_case(case):
    """-> (system arrays, [dict of results per rank])."""
    from atomsmm_amd.testing import tip3p_box
    c = tip3p_box(case['nside']) if case['density'] is None else tip3p_box(case['nside'], density=case['density'])
    if case['world'] == 1:
        return c, [_run(case, c)]
    from atomsmm_amd.engine import LocalWorld
    return c, LocalWorld(case['world']).run(lambda rank: _run(case, c))


FORCES = ('f1', 'f2', 'f1_moved', 'f2_moved', 'f1_squeezed', 'f2_squeezed')


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
            elif k.startswith('error_'):
                keep['r%d_%s' % (r, k)] = np.array(v)
    return keep


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'build_loops_%s.npz' % name)


def print_events(name, case):
    for second in ([False, True] if case['then'] else [False]):
        if case['world'] > 1:
            continue          # (a slice's parts follow another rule; its paths are those of the whole box's cases)
        ev = case_events(case, second)
        print(name, case['then'] if second else 'first', {k: (sorted(v) if isinstance(v, set) else v) for k, v in ev.items()}, flush=True)


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--events':
        for name in (args[1:] or sorted(CASES)):
            print_events(name, CASES[name])
        sys.exit(0)
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'          # (before the library is loaded: torch brings its own HIP runtime)
    from atomsmm_amd import backend
    print('kernel revision', backend.kernel_revision())
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
            print(name, 'rank', r, {k: (np.shape(v) if k in FORCES else (v if isinstance(v, str) else v.item())) for k, v in out.items()}, flush=True)
            assert all(np.all(np.isfinite(out[k])) for k in FORCES if k in out)
        print_events(name, CASES[name])
        print(name, '%.0f KB' % (os.path.getsize(path) / 1024.0), flush=True)
