#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_lookup_offset.py: what the molecule-row pair kernels compute must not depend on whether a
look-up subtracts the zone's base interval from the raw interval and adds the table's address, or adds a per-zone offset that holds
both (csrc/pair_tab.h: amm_tab_fetch_pass), nor on whether the guest of a fused pass multiplies its charge product by a factor of
exactly 1.0.

    python scripts/record_lookup_offset_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/lookup_offset_<case>.npz (or DIR/..., fp64) as scripts/record_zero_slot_goldens.py does: the group-1 (near) and
group-2 (outer) forces of one evaluation and positions and velocities after 6 outer steps of RESPA [4, 2, 1] -- of every atom for
the 1 536-atom boxes, of a seeded choice of 512 atoms for the larger one -- and, per array, the SHA-256 of ALL atoms' bytes.  The
'discount' case keeps the group-2 force of one fused launch whose guest carries the opposite sign (FarNonbondedForce: gfac = -1).
The files in the repository were recorded by the build of the commit BEFORE the zone offsets (kernel revision r09-zeroslot); the
test asks for the same bits.

The placements (placements()): an atom of one molecule is put where its r^2 from an atom of another is a chosen double -- the two ends
of each zone offset (first interval of zone A, last interval a counting pair reads in zone B) and the two sides of the zone boundary
(w = r^2 x scale = 1 and the double below it), for the Coulomb table (an oxygen-hydrogen pair) and the site-site table (two
oxygens), of the near and of the outer force."""
import importlib.util
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
_spec = importlib.util.spec_from_file_location('record_zero_slot_goldens', os.path.join(ROOT, 'scripts', 'record_zero_slot_goldens.py'))
Z = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(Z)
T, P = Z.T, Z.P

TWO = Z.TWO
STEPS = Z.STEPS
KEYS = Z.KEYS
TAB_SHIFT, PER_OCTAVE = 13, 128          # csrc/pair_tab.h: AMM_TAB_SHIFT, AMM_TAB_PER_OCTAVE

# the cases of scripts/record_zero_slot_goldens.py that the issue names are run again under this file's names; the rest is new
CASES = {
    'box8_fused': dict(nside=8, change=None, options=(), same_f1='box8_two_launches'),
    'box8_two_launches': dict(nside=8, change=None, options=TWO, same_f1='box8_fused'),
    'box17_fused': dict(nside=17, change=None, options=(), same_f1='box17_two_launches'),
    'box17_two_launches': dict(nside=17, change=None, options=TWO, same_f1='box17_fused'),
    'table_ends': dict(nside=8, change='ends', options=()),                        # fused: pairs below the outer table are redone
    'table_ends_two_launches': dict(nside=8, change='ends', options=TWO),           # the near table's own first interval is read
    'zone_boundary': dict(nside=8, change='boundary', options=(), same_f1='zone_boundary_two_launches'),
    'zone_boundary_two_launches': dict(nside=8, change='boundary', options=TWO, same_f1='zone_boundary'),
    'cutoff_edges': dict(nside=8, change='edges', options=(), same_f1='cutoff_edges_two_launches'),
    'cutoff_edges_two_launches': dict(nside=8, change='edges', options=TWO, same_f1='cutoff_edges'),
    'pushed_water': dict(nside=8, change='push', options=(), same_f1='pushed_water_two_launches'),
    'pushed_water_two_launches': dict(nside=8, change='push', options=TWO, same_f1='pushed_water'),
    'neutral_hydrogens': dict(nside=8, change='q0', options=(), same_f1='neutral_hydrogens_two_launches'),
    'neutral_hydrogens_two_launches': dict(nside=8, change='q0', options=TWO, same_f1='neutral_hydrogens'),
    'lattice_outside': dict(nside=8, change='lattice', options=()),
}
for _case in CASES.values():
    _case['outer'] = 'damped'


# ------------------------------------------------------------------------------------------------ the tables, as pair_tab.h lays them out
def _hi32(w):
    return struct.unpack('<Q', struct.pack('<d', w))[0] >> 32


def table_layout(rkink, rc, fine, site_sigma):
    """The intervals of a force's tables (csrc/pair_tab.h: amm_build_coulomb_table): r_kink the radius where the switching function
    starts, `fine` the refinement level of zone B (amm_pair_table_check reports it)."""
    scale = 1.0 / (rkink * rkink)
    octaves = max(3, min(10, int(np.ceil(2.0 * np.log2(rkink / 0.115)))))
    lay = dict(scale=scale, shiftB=TAB_SHIFT - fine, nA=octaves * PER_OCTAVE)
    lay['r2min'] = float(np.ldexp(1.0, -octaves)) / scale * (1.0 + 1e-12)
    lay['baseA'] = _hi32(float(np.ldexp(1.0, -octaves))) >> TAB_SHIFT
    lay['rawB_minus_nA'] = (_hi32(1.0) >> lay['shiftB']) - lay['nA']
    lay['nint'] = lay['nA'] + ((_hi32(rc * rc * scale * (1.0 + 1e-12)) >> lay['shiftB']) - (_hi32(1.0) >> lay['shiftB'])) + 2
    w0 = 0.49 * site_sigma * site_sigma * scale
    lay['ss_first'] = max(0, min((_hi32(w0) >> TAB_SHIFT) - lay['baseA'], lay['nA']))
    lo = struct.unpack('<d', struct.pack('<Q', ((lay['baseA'] + lay['ss_first']) << TAB_SHIFT) << 32))[0]
    lay['ss_r2min'] = lo / scale * (1.0 + 1e-12)
    return lay


def interval_of(lay, r2):
    """-> (w, interval) of r2 as the kernels form them (amm_tab_fetch_pass), without a clamp."""
    w = r2 * lay['scale']
    hi = _hi32(w)
    above = hi >= 0x3FF00000
    return w, (hi >> (lay['shiftB'] if above else TAB_SHIFT)) - (lay['rawB_minus_nA'] if above else lay['baseA'])


def r2_with_w(lay, w_want):
    """The double r2 with r2 x scale == w_want in fp64."""
    r2 = w_want / lay['scale']
    for _ in range(8):
        w = r2 * lay['scale']
        if w == w_want:
            return float(r2)
        r2 = float(np.nextafter(r2, np.inf if w < w_want else -np.inf))
    raise AssertionError('no r2 with w = %r' % w_want)


def layouts(fine_near, fine_outer):
    """The near force's (force switch 0.7 / 0.5 nm) and the outer force's (damped 2.9 / 1.0 / 0.9) tables of the TIP3P box."""
    return dict(near=table_layout(0.5, Z.RC_NEAR, fine_near, T.SIGMA_O), outer=table_layout(0.9, Z.RC_OUTER, fine_outer, T.SIGMA_O))


def fines():
    """Refinement level of zone B of the two forces' tables, from the library's host-side builder (no GPU)."""
    from atomsmm_amd import backend as B
    site = dict(site_sigma=T.SIGMA_O, site_eps=0.635968, site_q=-0.834)
    near = B.pair_table_check(B.pair_desc(B.NEAR_FSWITCH, Z.RC_NEAR, rc0=Z.RC_NEAR, rs0=0.5), **site)
    outer = B.pair_table_check(B.pair_desc(B.DAMPED, Z.RC_OUTER, rswitch=0.9, alpha=2.9, degree=1), **site)
    return near, outer


def _up(x, k=2):
    for _ in range(k):
        x = float(np.nextafter(x, np.inf))
    return x


def placements(change, lay):
    """-> [(name, atom of the anchor molecule, atom of the moved molecule, wanted r^2, table, site pair)]: 0 = oxygen, 1 = first hydrogen."""
    out = []
    for which in ('near', 'outer'):
        L = lay[which]
        rc2 = (Z.RC_NEAR if which == 'near' else Z.RC_OUTER) ** 2
        if change == 'ends':
            out.append((which + '_coulomb_first', 0, 1, _up(L['r2min']), which, False))
            out.append((which + '_site_first', 0, 0, _up(L['ss_r2min']), which, True))
            out.append((which + '_coulomb_last', 0, 1, float(np.nextafter(rc2, 0.0)), which, False))
            out.append((which + '_site_last', 0, 0, float(np.nextafter(rc2, 0.0)), which, True))
        if change == 'boundary':
            for tag, w in (('at', 1.0), ('below', float(np.nextafter(1.0, 0.0)))):
                out.append(('%s_coulomb_w1_%s' % (which, tag), 0, 1, r2_with_w(L, w), which, False))
                out.append(('%s_site_w1_%s' % (which, tag), 0, 0, r2_with_w(L, w), which, True))
    return out


def choose_pairs(c, wanted):
    """For every placement the pair of molecules that needs the shortest move (the liquid around it stays what it was), each
    molecule once: -> [(anchor molecule, moved molecule)] (as edge_pairs of scripts/record_zero_slot_goldens.py, for any atoms)."""
    x, L = c['positions'], c['box']
    used, out = set(), []
    for _, ai, aj, want, _, _ in wanted:
        target = x[ai::3] + np.array([np.sqrt(want), 0.0, 0.0])
        d = np.sqrt(((x[aj::3][None, :, :] - target[:, None, :]) ** 2).sum(-1))          # [anchor, mover]: no periodic image wanted
        inside = (target[:, 0] < L[0] - 0.2) & (x[ai::3][:, 0] > 0.2) & (x[ai::3][:, 2] > 0.2) & (x[ai::3][:, 2] < L[2] - 0.2)
        d[~inside, :] = np.inf
        for m in used:
            d[m, :] = np.inf
            d[:, m] = np.inf
        np.fill_diagonal(d, np.inf)
        i, j = np.unravel_index(int(np.argmin(d)), d.shape)
        used.update((int(i), int(j)))
        out.append((int(i), int(j)))
    return out


def make_system(case, lay=None):
    if case['change'] not in ('ends', 'boundary'):
        return Z.make_system(case)
    from atomsmm_amd.testing import tip3p_box
    if lay is None:
        near, outer = fines()
        lay = layouts(near['fine'], outer['fine'])
    c = tip3p_box(case['nside'])
    wanted = placements(case['change'], lay)
    pairs = choose_pairs(c, wanted)
    x = c['positions'].copy()
    for (name, ai, aj, want, _, _), (i, j) in zip(wanted, pairs):
        xi = x[3 * i + ai]
        target = Z.place_at_r2(xi, want)
        shift = target - x[3 * j + aj]
        x[3 * j:3 * j + 3] += shift
        x[3 * j + aj] = target
        assert Z.r2_of(float(target[0]) - float(xi[0]), float(target[2]) - float(xi[2])) == want and target[1] == xi[1], name
    c['positions'] = x
    c['placed'] = [(name, 3 * i + ai, 3 * j + aj, want, which, site) for (name, ai, aj, want, which, site), (i, j) in zip(wanted, pairs)]
    return c


def run_case(case):
    """-> (system arrays, dict f1 f2 x v, info): as scripts/record_zero_slot_goldens.py, with this file's systems."""
    c = make_system(case)
    context, integrator = T.build_context(case, c)
    eng = context._engine
    out = {}
    out['f1'], out['f2'] = P.group_forces(context)
    near, outer = eng.pair_force_ids(1)[0], eng.pair_force_ids(2)[0]
    info = dict(padding=eng.ctx.pair_row_padding(outer))
    integrator.step(STEPS)
    if hasattr(eng.ctx, 'pair_guest_factor'):
        info['guest_factor'] = eng.ctx.pair_guest_factor(near)
    st = context.getState(getPositions=True, getVelocities=True)
    out['x'] = st.getPositions(asNumpy=True)._value.copy()
    out['v'] = st.getVelocities(asNumpy=True)._value.copy()
    info.update(near=eng.ctx.pair_stats(near), outer=eng.ctx.pair_stats(outer), run=eng.ctx.run_stats())
    eng.ctx.check()
    return c, out, info


def run_discount(nside=8):
    """One force-only evaluation of FarNonbondedForce (total + discount, forces.py:710-724) on the TIP3P box with molecule rows: the
    discount -- a near force of sign -1 guarded by step(rc0 - r) -- rides on the total's walk as the guest of a fused pass over a
    reaction-field host, gfac = -1.  -> (system arrays, group-2 force, info)."""
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.testing import system_from_arrays, tip3p_box
    c = tip3p_box(nside)
    system = system_from_arrays(c, nonbondedMethod='CutoffPeriodic')
    nbforce = atomsmm.hijackForce(system, atomsmm.findNonbondedForce(system))
    inner = atomsmm.NearNonbondedForce(7.0 * unit.angstroms, 5.0 * unit.angstroms, 'force-switch')
    inner.importFrom(nbforce).addTo(system)
    outer = atomsmm.FarNonbondedForce(inner, 10 * unit.angstroms, 9.0 * unit.angstroms).setForceGroup(2)
    outer.importFrom(nbforce).addTo(system)
    integrator = openmm.CustomIntegrator(0.001)
    integrator.addComputePerDof('v', 'v + dt*f2/m')          # a force-only evaluation of group 2
    context = openmm.Context(system, integrator, openmm.Platform.getPlatformByName('HIP'), {'Option.cluster': '1'})
    context.setPositions(c['positions'] * unit.nanometers)
    eng = context._engine
    total, discount = eng.pair_force_ids(2)
    integrator.step(1)
    info = dict(total=eng.ctx.pair_stats(total), discount=eng.ctx.pair_stats(discount))
    if hasattr(eng.ctx, 'pair_guest_factor'):
        info['guest_factor'] = eng.ctx.pair_guest_factor(discount)
    eng.ctx.check()
    return c, eng._buffers['f2'].cpu().numpy().copy(), info


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'lookup_offset_%s.npz' % name)


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
    for name in (args or sorted(CASES) + ['discount']):
        if name == 'discount':
            c, f2, info = run_discount()
            path = golden_path(name, where)
            np.savez_compressed(path, f2=f2, sha_f2=np.array(Z.digest(f2)))
            print(name, '%.0f KB' % (os.path.getsize(path) / 1024.0), {k: info['discount'][k] for k in ('list_kind', 'rode_along', 'has_site_table')},
                  info.get('guest_factor'), flush=True)
            assert np.all(np.isfinite(f2))
            continue
        c, out, info = run_case(CASES[name])
        path = golden_path(name, where)
        keep = P.golden_atoms(len(out['x']))
        np.savez_compressed(path, **{k: np.asarray(out[k], dtype=np.float64)[keep] for k in KEYS},
                            **{'sha_' + k: np.array(Z.digest(out[k])) for k in KEYS})
        print(name, '%.0f KB' % (os.path.getsize(path) / 1024.0), 'padding (lane-trips, entries)', info['padding'],
              {k: info['near'][k] for k in ('list_kind', 'rode_along', 'has_site_table', 'lanes_per_atom')},
              'epilogues', info['run']['epilogues'], info.get('guest_factor'), flush=True)
        for p in c.get('placed', ()):
            print('   ', p, flush=True)
        assert np.all(np.isfinite(out['x'])) and np.all(np.isfinite(out['f2']))
