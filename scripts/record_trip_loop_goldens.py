#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_trip_loop.py: what the molecule-row pair kernels compute must not depend on which of their
arguments travel in scalar registers, on how a pair's lane conditions are combined, or on whether a sum with an exact zero is formed.

    python scripts/record_trip_loop_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/trip_loop_<case>.npz (or DIR/..., fp64): the group-1 and group-2 forces of one evaluation and positions and
velocities after 6 outer steps of RESPA [4, 2, 1] -- of every atom for the 1 536-atom boxes, of a seeded choice of 512 atoms for the
larger one (golden_atoms of scripts/record_pair_prologue_goldens.py); cases with `direct` also keep the two forces of ONE fused
launch of the pair forces alone (near force as guest of the outer force's walk, no step program, no epilogue: fd1, fd2).  The
files in the repository were recorded by the build of the commit BEFORE the trip loop was reworked (kernel revision r06-prologue);
the test asks for the same bits.  The cases are those the cases of record_pair_prologue_goldens.py do not reach."""
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

SIGMA_O = 0.315075
TABLE_END = 0.115          # nm: the lower end of every Coulomb table (csrc/pair_tab.h: amm_build_coulomb_table)

# name -> box side, what is done to the TIP3P box, the outer force (group 2), library options
#   outer: 'damped' DampedSmoothedForce(2.9, 1.0, 0.9) as in the bench; 'pme' / 'rf' the NonbondedForce of RESPASystem as it is
#   (Ewald direct space / reaction field: NONBONDED hosts, whose step-boundary pass carries no epilogue)
CASES = {
    'pushed_water': dict(nside=8, change='push', outer='damped', options=()),            # (a) analytic branch, host and guest
    'neutral_hydrogens': dict(nside=8, change='q0', outer='damped', options=()),         # (b) signed zeros on the site-table path
    'two_site_classes': dict(nside=8, change='eps', outer='damped', options=()),         # (c) no site tables: the guest keeps its LJ sum
    'ewald_direct_host': dict(nside=8, change=None, outer='pme', options=(), direct=True),      # (d)
    'reaction_field_host': dict(nside=8, change=None, outer='rf', options=(), direct=True),     # (d)
    'launches_of_their_own': dict(nside=8, change=None, outer='damped', options=(('fuse_epilogue', 0),)),      # (e)
    'box17_interior': dict(nside=17, change=None, outer='damped', options=()),           # (f) tasks without a periodic image
}
STEPS = 6


def make_system(case):
    """The arrays of the case's box (atomsmm_amd.testing.tip3p_box, changed as the case says)."""
    from atomsmm_amd.testing import tip3p_box
    c = tip3p_box(case['nside'])
    if case['change'] == 'push':
        # the molecule nearest to the spot is moved, as it is, to where its oxygen sits 0.2 nm from the oxygen of molecule 0 on the
        # line through that molecule's first hydrogen: O-O 0.2 nm < 0.7 sigma = 0.2206 nm, H(0)-O 0.2 - 0.0957 = 0.104 nm < 0.115 nm
        x = c['positions'].copy()
        u = (x[1] - x[0]) / np.linalg.norm(x[1] - x[0])
        spot = x[0] + 0.2 * u
        d = x[3::3] - spot
        d -= c['box'] * np.round(d / c['box'])
        j = 1 + int(np.argmin((d * d).sum(-1)))
        x[3 * j:3 * j + 3] -= d[j - 1]
        c['positions'] = x
    elif case['change'] == 'q0':
        q = c['charge'].copy()
        mol = np.arange(len(q) // 3)
        q[3 * mol[mol % 5 == 0] + 1] = 0.0          # first hydrogen of every fifth molecule
        q[3 * mol[mol % 7 == 0] + 2] = 0.0          # second hydrogen of every seventh
        c['charge'] = q
    elif case['change'] == 'eps':
        e = c['epsilon'].copy()
        mol = np.arange(len(e) // 3)
        e[3 * mol[mol % 3 == 0]] *= 1.21            # a second class of oxygens: the force has no site-site table
        c['epsilon'] = e
    return c


def closest_pairs(c):
    """-> (smallest O-H distance between different molecules, smallest O-O distance), minimum image."""
    x, L = c['positions'], c['box']
    o, h = x[0::3], np.concatenate([x[1::3], x[2::3]])
    mol_h = np.concatenate([np.arange(len(o)), np.arange(len(o))])

    def dist(a, b):
        d = a[:, None, :] - b[None, :, :]
        d -= L * np.round(d / L)
        return np.sqrt((d * d).sum(-1))
    doh = dist(o, h)
    doh[mol_h[None, :] == np.arange(len(o))[:, None]] = np.inf
    doo = dist(o, o)
    np.fill_diagonal(doo, np.inf)
    return float(doh.min()), float(doo.min())


def build_context(case, c):
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.testing import system_from_arrays
    system = system_from_arrays(c, nonbondedMethod='PME' if case['outer'] == 'pme' else 'CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    if case['outer'] == 'damped':
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
    return context, integrator


def direct_descs(case):
    """Oracle descriptions of the two pair forces of a `direct` case: the near force and the outer NonbondedForce's pair part."""
    from oracle import oracle as O
    dn = O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5)
    if case['outer'] == 'pme':
        dh = O.desc(O.NONBONDED, rc=1.0, rswitch=0.9, alpha=2.628260884878466, flags=O.COULOMB_EWALD | O.SWITCH)
    else:
        eps_rf = 78.3
        dh = O.desc(O.NONBONDED, rc=1.0, rswitch=0.9, flags=O.SWITCH | O.COULOMB_RF, krf=(eps_rf - 1) / (2 * eps_rf + 1),
                    crf=3 * eps_rf / (2 * eps_rf + 1))
    return dn, dh


def run_direct(case, c):
    """One fused launch of the two pair forces alone, through the C-ABI: -> (near force, outer force, stats of both)."""
    import torch
    from atomsmm_amd import backend as B
    n = len(c['positions'])
    ctx = B.HipContext(n, c['box'])
    ids = []
    for d in direct_descs(case):
        desc = B.pair_desc(d.family, d.rc, rc0=d.rc0, rs0=d.rs0, rswitch=d.rswitch, alpha=d.alpha, degree=d.degree, flags=d.flags,
                           sign=d.sign, Kc=d.Kc, krf=d.krf, crf=d.crf)
        ids.append(ctx.pair_create(desc, c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'], skin=-1.0))
    fn, fh = ids
    ctx.pair_share_list(fn, fh)

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')
    x, v, m = dev(c['positions']), dev(c['velocities']), dev(c['mass'])
    bufs = [torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda') for _ in range(2)]
    ctx.bind_state(x, v, m)
    ctx.bind_buffer(1, bufs[0])
    ctx.bind_buffer(2, bufs[1])
    ctx.group_define(1, 1, [fn])
    ctx.group_define(2, 2, [fh])
    ctx.run_ops([B.Op(B.OP_EVAL, 1, 0, 0, 0.0), B.Op(B.OP_EVAL, 2, 0, 0, 0.0)], 1)
    ctx.check()
    out = bufs[0].cpu().numpy().copy(), bufs[1].cpu().numpy().copy(), ctx.pair_stats(fn), ctx.pair_stats(fh)
    ctx.close()
    return out


def run_case(case):
    """-> (system arrays, dict of results).  f1, f2: one evaluation of groups 1 and 2; x, v: after STEPS outer steps; stats of the
    near force and of the list's owner; run_stats of the context; fd1, fd2 (cases with `direct`)."""
    c = make_system(case)
    context, integrator = build_context(case, c)
    eng = context._engine
    out = {}
    out['f1'], out['f2'] = P.group_forces(context)
    integrator.step(STEPS)
    st = context.getState(getPositions=True, getVelocities=True)
    out['x'] = st.getPositions(asNumpy=True)._value.copy()
    out['v'] = st.getVelocities(asNumpy=True)._value.copy()
    info = dict(near=eng.ctx.pair_stats(eng.pair_force_ids(1)[0]), outer=eng.ctx.pair_stats(eng.pair_force_ids(2)[0]), run=eng.ctx.run_stats())
    eng.ctx.check()
    if case.get('direct'):
        out['fd1'], out['fd2'], info['direct_near'], info['direct_outer'] = run_direct(case, c)
    return c, out, info


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'trip_loop_%s.npz' % name)


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
        np.savez_compressed(path, **{k: np.asarray(v, dtype=np.float64)[keep] for k, v in out.items() if k in ('f1', 'f2', 'x', 'v')})
        if 'fd1' in out:          # (a file of its own: every golden stays below 150 KB)
            np.savez_compressed(golden_path(name + '_direct', where), fd1=out['fd1'], fd2=out['fd2'])
        print(name, {k: np.shape(v) for k, v in out.items()}, '%.0f KB' % (os.path.getsize(path) / 1024.0),
              'closest O-H %.4f O-O %.4f' % closest_pairs(c) if len(out['x']) <= 1536 else '', flush=True)
        for key in sorted(info):
            print('   ', key, {k: info[key][k] for k in sorted(info[key]) if k in
                               ('list_kind', 'rode_along', 'has_site_table', 'epilogues', 'n_builds', 'lanes_per_atom')}, flush=True)
        assert np.all(np.isfinite(out['x'])) and np.all(np.isfinite(out['f2']))
