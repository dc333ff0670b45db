#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_zero_slot.py: what the molecule-row pair kernels compute must not depend on whether a pair
that does not count (beyond the cutoff, a padding lane, below the table) has its force thrown away by a select or reads a slot of
zeros in LDS, nor on whether the interval of a counting pair is clamped.

    python scripts/record_zero_slot_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/zero_slot_<case>.npz (or DIR/..., fp64): the group-1 (near) and group-2 (outer) forces of one evaluation and
positions and velocities after 6 outer steps of RESPA [4, 2, 1] -- of every atom for the 1 536-atom boxes, of a seeded choice of 512
atoms for the larger one (golden_atoms of scripts/record_pair_prologue_goldens.py) -- and, per array, the SHA-256 of ALL atoms'
bytes (so that a sign of zero or a bit of any atom shows).  The files in the repository were recorded by the build of the commit
BEFORE the zero slot (kernel revision r08-buildtabs); the test asks for the same bits."""
import hashlib
import importlib.util
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
_spec = importlib.util.spec_from_file_location('record_trip_loop_goldens', os.path.join(ROOT, 'scripts', 'record_trip_loop_goldens.py'))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
P = T.P

RC_NEAR, RC_OUTER, SKIN = 0.7, 1.0, 0.1
LATTICE_A = 1.2            # nm: spacing of the 'lattice_outside' case
TWO = (('fuse_rows', 0),)  # the two forces of the shared list as launches of their own (no fused step-boundary pass)

# name -> box side, what is done to the TIP3P box (make_system), library options, the case whose near force must have the same bits
CASES = {
    'box8_fused': dict(nside=8, change=None, options=(), same_f1='box8_two_launches'),             # per-pair image loop
    'box8_two_launches': dict(nside=8, change=None, options=TWO, same_f1='box8_fused'),
    'box17_fused': dict(nside=17, change=None, options=(), same_f1='box17_two_launches'),          # interior and image/molecule tasks
    'box17_two_launches': dict(nside=17, change=None, options=TWO, same_f1='box17_fused'),
    'box8_lanes8': dict(nside=8, change=None, options=(('lanes_per_row', 8),)),                    # rows of ~57 / ~150 entries at 8 lanes
    'cutoff_edges': dict(nside=8, change='edges', options=(), same_f1='cutoff_edges_two_launches'),
    'cutoff_edges_two_launches': dict(nside=8, change='edges', options=TWO, same_f1='cutoff_edges'),
    'pushed_water': dict(nside=8, change='push', options=(), same_f1='pushed_water_two_launches'),  # analytic redo inside ordinary trips
    'pushed_water_two_launches': dict(nside=8, change='push', options=TWO, same_f1='pushed_water'),
    'neutral_hydrogens_two_launches': dict(nside=8, change='q0', options=TWO),                     # q_i q_j = 0 and < 0
    'lattice_outside': dict(nside=8, change='lattice', options=()),                                # listed partners, none within a cutoff
}
for _case in CASES.values():
    _case['outer'] = 'damped'
STEPS = T.STEPS


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def _exact_diff(a, b):
    d = a - b
    return d if Fraction(a) - Fraction(b) == Fraction(d) else None


def r2_of(dx, dz):
    """r^2 of a pair displaced by (dx, 0, dz) as fp64 arithmetic gives it whichever way the three products are contracted into FMAs:
    dx * dx rounded, then + dz * dz with one rounding (dy = 0 adds nothing)."""
    return float(Fraction(dx * dx) + Fraction(dz) * Fraction(dz))


def place_at_r2(xi, want):
    """-> position (x, y, z) of an oxygen such that its r^2 from the oxygen at xi is exactly `want` (r2_of): displaced along x by
    about sqrt(want), along z by what the last ulps need, not at all along y.  Differences of the coordinates are exact."""
    xt = float(xi[0]) + float(np.sqrt(want))
    for k in range(0, -12, -1):
        xj = _step(xt, k)
        dx = _exact_diff(xj, float(xi[0]))
        if dx is None or not (dx * dx < want):
            continue
        dz0 = float(np.sqrt(want - dx * dx))
        for m in range(-4, 5):
            zj = _step(float(xi[2]) + dz0, m)
            dz = _exact_diff(zj, float(xi[2]))
            if dz is not None and r2_of(dx, dz) == want:
                return np.array([xj, float(xi[1]), zj])
    raise AssertionError('no position with r2 = %r' % want)


def edge_pairs(c):
    """The four placements of the 'edges' case: (anchor molecule, molecule to move, wanted r^2) -- r^2 = rc^2 (does not count:
    r2 < rc2 fails) and the last double below it (counts: the top of the table), for the near and for the outer cutoff.  Of all pairs
    of molecules the one that needs the shortest move is taken (the liquid around it stays what it was), each molecule once."""
    x, L = c['positions'][0::3], c['box']
    wants = [RC_NEAR * RC_NEAR, float(np.nextafter(RC_NEAR * RC_NEAR, 0.0)), RC_OUTER * RC_OUTER, float(np.nextafter(RC_OUTER * RC_OUTER, 0.0))]
    used, out = set(), []
    for want in wants:
        target = x + np.array([np.sqrt(want), 0.0, 0.0])
        d = np.sqrt(((x[None, :, :] - target[:, None, :]) ** 2).sum(-1))          # [anchor, mover]: no periodic image wanted
        inside = (target[:, 0] < L[0] - 0.2) & (x[:, 2] > 0.2) & (x[:, 2] < L[2] - 0.2)
        d[~inside, :] = np.inf
        for m in used:
            d[m, :] = np.inf
            d[:, m] = np.inf
        np.fill_diagonal(d, np.inf)
        i, j = np.unravel_index(int(np.argmin(d)), d.shape)
        used.update((int(i), int(j)))
        out.append((int(i), int(j), want))
    return out


def make_system(case):
    from atomsmm_amd.testing import tip3p_box
    if case['change'] in (None, 'push', 'q0', 'eps'):
        return T.make_system(case)
    c = tip3p_box(case['nside'])
    x = c['positions'].copy()
    if case['change'] == 'edges':
        for anchor, j, want in edge_pairs(c):
            xi = x[3 * anchor]
            target = place_at_r2(xi, want)
            shift = target - x[3 * j]
            x[3 * j + 1:3 * j + 3] += shift
            x[3 * j] = target
            assert 0.0 < target[0] < c['box'][0] and 0.0 < target[2] < c['box'][2]
            assert r2_of(float(x[3 * j, 0]) - float(xi[0]), float(x[3 * j, 2]) - float(xi[2])) == want and x[3 * j, 1] == xi[1]
    elif case['change'] == 'lattice':
        # the molecules as they are (orientation, geometry), their oxygens on a cubic lattice of LATTICE_A: nearest neighbours are
        # listed (first atoms closer than list radius + twice the molecule's extent: 1.1 + 0.29 nm) and no atom pair is within
        # the outer cutoff (1.2 - 2 x 0.0957 = 1.0086 nm).  In the lower half of the box (iz < 4) every second molecule along x
        # is moved 0.3 nm towards its neighbour: pairs at 0.9 nm, inside the outer cutoff and in the near force's front part.
        n = case['nside']
        idx = np.arange(n ** 3)
        ix, iy, iz = idx // (n * n), (idx // n) % n, idx % n
        centre = (np.stack([ix, iy, iz], -1) + 0.5) * LATTICE_A
        centre[(ix % 2 == 1) & (iz < 4), 0] -= 0.3
        mol = x.reshape(-1, 3, 3)
        mol += (centre - mol[:, 0])[:, None, :]
        x = mol.reshape(-1, 3)
        c['box'] = np.full(3, n * LATTICE_A)
    c['positions'] = x
    return c


def lattice_far_molecules(case):
    """Molecules of the 'lattice' case all of whose listed partners are outside both cutoffs: the upper half of the box."""
    n = case['nside']
    return np.nonzero(np.arange(n ** 3) % n >= 4)[0]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def run_case(case):
    """-> (system arrays, dict f1 f2 x v, info): as scripts/record_trip_loop_goldens.py, with this file's systems."""
    c = make_system(case)
    context, integrator = T.build_context(case, c)
    eng = context._engine
    out = {}
    out['f1'], out['f2'] = P.group_forces(context)
    near, outer = eng.pair_force_ids(1)[0], eng.pair_force_ids(2)[0]
    info = dict(padding=eng.ctx.pair_row_padding(outer))
    integrator.step(STEPS)
    st = context.getState(getPositions=True, getVelocities=True)
    out['x'] = st.getPositions(asNumpy=True)._value.copy()
    out['v'] = st.getVelocities(asNumpy=True)._value.copy()
    info.update(near=eng.ctx.pair_stats(near), outer=eng.ctx.pair_stats(outer), run=eng.ctx.run_stats())
    eng.ctx.check()
    return c, out, info


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'zero_slot_%s.npz' % name)


KEYS = ('f1', 'f2', 'x', 'v')

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
        c, out, info = run_case(CASES[name])
        path = golden_path(name, where)
        keep = P.golden_atoms(len(out['x']))
        np.savez_compressed(path, **{k: np.asarray(out[k], dtype=np.float64)[keep] for k in KEYS},
                            **{'sha_' + k: np.array(digest(out[k])) for k in KEYS})
        print(name, '%.0f KB' % (os.path.getsize(path) / 1024.0), 'padding (lane-trips, entries)', info['padding'],
              {k: info['near'][k] for k in ('list_kind', 'rode_along', 'has_site_table', 'lanes_per_atom')},
              'epilogues', info['run']['epilogues'], flush=True)
        assert np.all(np.isfinite(out['x'])) and np.all(np.isfinite(out['f2']))
