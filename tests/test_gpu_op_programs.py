"""The op scheduler (csrc/run_ops.hip) on step programs that no propagator emits: programs that sit ON the guards of its six fusion
rules and of its two kinds of epilogue plan, structured random programs, resumption at every cursor, and the two modes.

Everything goes through backend.HipContext (no engine).  The check is the same for every program: two fresh contexts from one initial
state, one with amm_set_fuse_inner(1) and one with (0); in each a first amm_run_ops call evaluates every group, then the program
runs.  x, v, EVERY bound buffer and the lists' build counts must be equal bit for bit, everything finite, the atoms moved, amm_check
clean, the plain run's `scheduled` exactly n_ops * repeat - start, the fused run's per-rule counters (amm_run_rule_stats) what the
case's derivation says.  Where tests/ops_ref.py restates the fixture's forces and the program moves for at most 8 fs the plain
result is also held against that interpreter (1e-11 nm, 1e-9 nm/ps: the bounds of test_respa_ops_vs_oracle_trajectory).

Fixtures: W flexible TIP3P 8^3 (group 0 bonds + angles / slot 0, group 1 near force-switch / slot 1, group 2 damped outer / slot 2,
slot 3 scratch; the near force on the outer force's list, on a list of its own, and shared without site tables), L the chargeless
LJ fluid 12^3 (group 1 force-switch / slot 1, group 2 shifted / slot 2), C emim-BCN4 (group 0 bonds / slot 0, group 3 angles +
torsions / slot 1; components of up to 19 atoms; C5 = the same with option terms_from = 1), H heaq (group 0 = softcore small-group pair
force + every bond-list term / slot 0, terms_from = 1).

Counters are written p (plain path), r1..r6 (rules 1..6), off (evaluations offered a plan), epi (launches that carried one).  The
derivations stand next to the cases (CASES below); what the MI355X gave is in OBSERVED_ON_MI355X at the end of this docstring.

Not reachable, by the scheduler's own guards (so no case): deferred kicks meeting a non-kick at op 0 (rule 1 defers only when op 0 is a
KICK, and every repetition starts at op 0 or behind a wrapped plan, which consumed the closing kicks); `nk - 1 > AMM_MAX_PRE` in
plan_epilogue (its kick_run stops at AMM_MAX_PRE + 1 kicks: an eighth kick fails the KICK ; MOVE test of the pattern first -- case
dual-pre7); rule 1 with `swapped` set but f0_slot < 0 (rule 3 sets f0_slot before it swaps and nothing resets it inside a call).

Measured on an MI355X: the worst deviation of a plain run from tests/ops_ref.py over all 203 comparisons of this module (guards,
random programs, resumption; W, L, C, C5) is 8.9e-16 nm in the positions and 2.3e-13 nm/ps in the velocities, against the bounds of
1e-11 nm and 1e-9 nm/ps.  The whole module (173 tests) takes about 17 s.

OBSERVED_ON_MI355X -- the fused run's counters of every case of (a), then decisions fused / plain; each equals its derivation in CASES:
    W/kicks1-move                      p=1 r6=1                                      2 /  3
    W/kicks2-move                      p=1 r6=1                                      2 /  4
    W/kicks3-move                      p=1 r6=1                                      2 /  5
    W/kicks4-move                      p=1 r6=1                                      2 /  6
    W/kicks5-move                      p=1 r6=2                                      3 /  7
    W/kicks6-move                      p=1 r6=2                                      3 /  8
    W/kicks1-alone                     p=4                                           4 /  4
    W/kicks2-alone                     p=3 r6=1                                      4 /  5
    W/kicks3-alone                     p=3 r6=1                                      4 /  6
    W/kicks4-alone                     p=3 r6=1                                      4 /  7
    W/kicks5-alone                     p=4 r6=1                                      5 /  8
    W/kicks6-alone                     p=3 r6=2                                      5 /  9
    W/pre0-iter                        p=1 r2=1                                      2 /  5
    W/pre1-iter                        p=1 r2=1                                      2 /  6
    W/pre2-iter                        p=1 r2=1                                      2 /  7
    W/pre3-iter                        p=1 r2=1                                      2 /  8
    W/pre4-iter                        p=1 r2=1 r6=1                                 3 /  9
    W/pre5-iter                        p=1 r2=1 r6=1                                 3 / 10
    W/pre6-iter                        p=1 r2=1 r6=1                                 3 / 11
    W/pre0-iter3                       p=1 r2=1                                      2 / 13
    W/pre1-iter3                       p=1 r2=1                                      2 / 14
    W/pre2-iter3                       p=1 r2=1                                      2 / 15
    W/pre3-iter3                       p=1 r2=1                                      2 / 16
    W/pre0-bathed1                     p=1 r2=1                                      2 /  7
    W/pre0-bathed3                     p=1 r2=1                                      2 / 19
    W/pre1-bathed1                     p=1 r2=1                                      2 /  8
    W/pre1-bathed3                     p=1 r2=1                                      2 / 20
    W/pre2-bathed1                     p=1 r2=1                                      2 /  9
    W/pre2-bathed3                     p=1 r2=1                                      2 / 21
    W/pre3-bathed1                     p=1 r2=1                                      2 / 10
    W/pre3-bathed3                     p=1 r2=1                                      2 / 22
    W/pre4-bathed1                     p=1 r2=1 r6=1                                 3 / 11
    W/iter-closing-coef                p=1 r2=3                                      4 / 13
    W/iter-closing-buffer              p=3 r6=1                                      4 /  5
    W/trail1-r1                        p=2 r6=1                                      3 /  4
    W/trail1-r2                        p=3 r1=1 r6=2                                 6 /  8
    W/trail1-r3                        p=4 r1=2 r6=3                                 9 / 12
    W/trail2-r1                        p=1 r6=2                                      3 /  5
    W/trail2-r2                        p=2 r1=1 r6=3                                 6 / 10
    W/trail2-r3                        p=3 r1=2 r6=4                                 9 / 15
    W/trail3-r1                        p=1 r6=2                                      3 /  6
    W/trail3-r2                        p=2 r1=1 r6=3                                 6 / 12
    W/trail3-r3                        p=3 r1=2 r6=4                                 9 / 18
    W/trail4-r1                        p=1 r6=2                                      3 /  7
    W/trail4-r2                        p=2 r6=4                                      6 / 14
    W/trail4-r3                        p=3 r6=6                                      9 / 21
    W/trail-copy-safe-r2               p=5 r1=1 r6=2                                 8 / 12
    W/trail-copy-safe-r3               p=6 r1=2 r6=3                                11 / 18
    W/trail-copy-dest-read-r2          p=6 r6=2                                      8 / 10
    W/trail-copy-dest-read-r3          p=9 r6=3                                     12 / 15
    W/trail-copy-slot-v-r2             p=6 r6=2                                      8 / 10
    W/defer-meets-rule2-r2             r1=1 r2=2 r6=1                                4 / 12
    W/defer-meets-rule2-r3             r1=2 r2=3 r6=1                                6 / 18
    W/defer-meets-rule3-guard-r2       p=2 r1=1 r6=3                                 6 / 10
    W/defer3-run1-r2                   p=2 r1=1 r6=3                                 6 / 12
    W/defer2-run2-r2                   p=2 r1=1 r6=3                                 6 / 12
    W/defer3-run2-r2                   p=2 r1=1 r6=3                                 6 / 14
    W/defer2-run3-r2                   p=2 r1=1 r6=3                                 6 / 14
    W/dual-E2E1-plan                   p=1 r4=1 off=1 epi=1                          2 / 13
    W/dual-E1E2-plan                   p=1 r4=1 off=1 epi=1                          2 / 13
    W/dual-copy                        p=2 r2=1 r4=1                                 4 / 14
    W/dual-pre6                        p=1 r4=1 off=1 epi=1                          2 / 13
    W/dual-pre7                        p=1 r2=1 r4=1 r6=1                            4 / 14
    W-unshared/unshared-E2E1-plan      p=3 off=1 epi=1                               3 / 13
    W-nositetab/nositetab-E2E1-plan    p=1 r2=1 r4=1 off=1                           3 / 13
    W/wrapped-r1                       r2=1 r4=1 r6=1                                3 / 14
    W/wrapped-r2                       r2=1 r4=2 r6=1 off=1 epi=1                    4 / 28
    W/wrapped-r3                       r2=1 r4=3 r6=1 off=2 epi=2                    5 / 42
    L/vv1-r1                           p=2 r6=1                                      3 /  4
    L/vv1-r3                           p=4 r6=1 off=2 epi=2                          5 / 12
    L/vv2-r3                           p=3 r6=2 off=2 epi=2                          5 / 18
    L/vv4-r1                           p=1 r6=2                                      3 / 10
    L/vv4-r3                           p=3 r6=6                                      9 / 30
    L/vv5-r1                           p=2 r6=3                                      5 / 12
    L/vv5-r3                           p=4 r1=2 r6=9                                15 / 36
    L-nochargeless/vv1-r3-no-kernel    p=4 r1=2 r6=3 off=2                           9 / 12
    C/iter1                            p=1 r3=1                                      2 /  5
    C/iter2                            p=1 r3=2                                      3 /  9
    C/iter3                            p=1 r3=3                                      4 / 13
    C/odd-then-ops                     p=8 r3=1 r6=2                                11 / 16
    C/even-then-group3                 p=3 r3=2 r6=1                                 6 / 13
    C/group3-first                     p=3 r3=1 r6=1                                 5 /  9
    C/trailing-after-iter-r2           r3=2 r6=2                                     4 / 12
    C/EKKM-not-term-parallel           p=2 r6=1                                      3 /  5
    C5/EK                              p=3 r5=1                                      4 /  5
    C5/EKKM                            p=1 r5=1                                      2 /  5
    C5/E5K                             p=3 r5=1                                      4 /  8
    C5/EKMM                            p=2 r5=1                                      3 /  5
    H/EK                               p=3 r5=1                                      4 /  5
    H/EKKM                             p=1 r5=1                                      2 /  5
    H/E5K                              p=3 r5=1                                      4 /  8
    H/EKMM                             p=2 r5=1                                      3 /  5
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import ops_ref  # noqa: E402
from ops_ref import CB, CP, E, K, M, SLOT_V, SLOT_X  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

FS = 0.001                      # ps
POS_BOUND, VEL_BOUND = 1e-11, 1e-9
REF_HORIZON = 8 * FS + 1e-12
KEYS = ('p', 'r1', 'r2', 'r3', 'r4', 'r5', 'r6', 'off', 'epi')
OP_BATH = 7


def _backend():
    from atomsmm_amd import backend as B
    return B


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def X(**kw):
    """expected counters; what is not named is 0"""
    assert set(kw) <= set(KEYS)
    return {k: kw.get(k, 0) for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------- fixtures
class Rig:
    """A fixture: the arrays, how a context is furnished with its forces and groups, and (where ops_ref restates them) the same
    groups over the oracle."""

    def __init__(self, name, case, v0, slots, prologue, define, ref_groups, options=()):
        self.name, self.case, self.slots, self.prologue, self.define, self.ref_groups, self.options = \
            name, case, tuple(slots), prologue, define, ref_groups, tuple(options)
        self.x0 = np.ascontiguousarray(case['positions'], dtype=np.float64)
        self.v0 = np.ascontiguousarray(v0, dtype=np.float64)
        self.mass = np.ascontiguousarray(case['mass'], dtype=np.float64)
        self.n = len(self.x0)
        self._ref_start = None

    def ref_state(self):
        """the state behind the first call (every group evaluated) on the reference interpreter: computed once, handed out as copies"""
        if self._ref_start is None:
            self._ref_start = ops_ref.run(self.prologue, 1, ops_ref.new_state(self.x0, self.v0, self.mass, self.slots), self.ref_groups)
        s = self._ref_start
        return dict(x=s['x'].copy(), v=s['v'].copy(), mass=s['mass'], bufs={k: b.copy() for k, b in s['bufs'].items()})


def _pair(B, ctx, d, c):
    desc = B.pair_desc(d.family, d.rc, rc0=d.rc0, rs0=d.rs0, rswitch=d.rswitch, alpha=d.alpha, degree=d.degree, flags=d.flags,
                       sign=d.sign, Kc=d.Kc, krf=d.krf, crf=d.crf)
    return ctx.pair_create(desc, c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'])


def load_case(case):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', case + '.npz'))
    return {k: d[k] for k in d.files}


def _thermal(mass, seed):
    return np.random.default_rng(seed).normal(size=(len(mass), 3)) * np.sqrt(2.494 / mass)[:, None]


@functools.lru_cache(maxsize=None)
def rig(name):
    from atomsmm_amd.testing import lj_fluid, tip3p_box
    B = _backend()
    if name in ('W', 'W-unshared', 'W-nositetab'):
        c = tip3p_box(8)
        dn = O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5)
        dd = O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1)

        def define(ctx):
            bid = ctx.bonded_create()
            ctx.bonded_add_terms(bid, B.BOND_HARMONIC, c['bonds'], np.stack([c['bond_r0'], c['bond_k']], 1))
            ctx.bonded_add_terms(bid, B.ANGLE_HARMONIC, c['angles'], np.stack([c['angle_theta0'], c['angle_k']], 1))
            ctx.bonded_finalize(bid)
            nid, did = _pair(B, ctx, dn, c), _pair(B, ctx, dd, c)
            if name != 'W-unshared':
                ctx.pair_share_list(nid, did)
            ctx.group_define(0, 0, [bid]); ctx.group_define(1, 1, [nid]); ctx.group_define(2, 2, [did])
            return [nid, did]

        groups = {0: (0, ops_ref.oracle_forces(c, bonds=True, angles=True)), 1: (1, ops_ref.oracle_forces(c, pair=dn)),
                  2: (2, ops_ref.oracle_forces(c, pair=dd))}
        return Rig(name, c, c['velocities'], (0, 1, 2, 3), [E(2), E(1), E(0), CP(3, 1)], define, groups,
                   options=(('site_tab', 0),) if name == 'W-nositetab' else ())
    if name in ('L', 'L-nochargeless'):
        c = lj_fluid(12)
        d1 = O.desc(O.NEAR_FSWITCH, rc=0.85, rc0=0.85, rs0=0.765)
        d2 = O.desc(O.NEAR_SHIFT, rc=0.8, rc0=0.8, rs0=0.7)

        def define(ctx):
            a, b = _pair(B, ctx, d1, c), _pair(B, ctx, d2, c)
            ctx.group_define(1, 1, [a]); ctx.group_define(2, 2, [b])
            return [a, b]

        groups = {1: (1, ops_ref.oracle_forces(c, pair=d1)), 2: (2, ops_ref.oracle_forces(c, pair=d2))}
        return Rig(name, c, _thermal(c['mass'], 4), (1, 2, 3), [E(1), E(2), CP(3, 2)], define, groups,
                   options=(('chargeless', 0),) if name == 'L-nochargeless' else ())
    if name in ('C', 'C5'):
        c = load_case('emim_BCN4_Jiung2014')

        def define(ctx):
            b0 = ctx.bonded_create()
            ctx.bonded_add_terms(b0, B.BOND_HARMONIC, c['bonds'], np.stack([c['bond_r0'], c['bond_k']], 1), periodic=True)
            ctx.bonded_finalize(b0)
            b3 = ctx.bonded_create()
            ctx.bonded_add_terms(b3, B.ANGLE_HARMONIC, c['angles'], np.stack([c['angle_theta0'], c['angle_k']], 1), periodic=True)
            ctx.bonded_add_terms(b3, B.TORSION_PERIODIC, c['torsions'], np.stack([c['torsion_n'].astype(np.float64), c['torsion_phase'], c['torsion_k']], 1),
                                 periodic=True)
            ctx.bonded_finalize(b3)
            ctx.group_define(0, 0, [b0]); ctx.group_define(3, 1, [b3])
            return []

        groups = {0: (0, ops_ref.oracle_forces(c, bonds=True, periodic=True)), 3: (1, ops_ref.oracle_forces(c, angles=True, torsions=True, periodic=True))}
        return Rig(name, c, _thermal(c['mass'], 5), (0, 1, 3), [E(0), E(3), CP(3, 1)], define, groups,
                   options=(('terms_from', 1 if name == 'C5' else 100000),))
    if name == 'H':
        c = load_case('hydroxyethylaminoanthraquinone-in-water')
        codes = np.where(c['resname'] == 'aaa', 1.0, 2.0)
        assert 0 < int((codes == 1.0).sum()) <= 128

        def define(ctx):
            # SolvationSystem's softcore force (one interaction group: solute x everything else) as the engine hands it over: the
            # codes in the charge slot, lambda in alpha, Kc = 1
            desc = B.pair_desc(B.SOFTCORE, 1.0, rswitch=0.9, alpha=0.7, flags=B.SWITCH, Kc=1.0)
            pid = ctx.pair_create(desc, codes, c['sigma'], c['epsilon'], None)
            bid = ctx.bonded_create()
            ctx.bonded_add_terms(bid, B.BOND_HARMONIC, c['bonds'], np.stack([c['bond_r0'], c['bond_k']], 1), periodic=True)
            ctx.bonded_add_terms(bid, B.ANGLE_HARMONIC, c['angles'], np.stack([c['angle_theta0'], c['angle_k']], 1), periodic=True)
            ctx.bonded_add_terms(bid, B.TORSION_PERIODIC, c['torsions'], np.stack([c['torsion_n'].astype(np.float64), c['torsion_phase'], c['torsion_k']], 1),
                                 periodic=True)
            ctx.bonded_finalize(bid)
            ctx.group_define(0, 0, [pid, bid])
            return []

        return Rig(name, c, _thermal(c['mass'], 6), (0, 3), [E(0), CP(3, 0)], define, None, options=(('terms_from', 1),))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- running
def as_ops(B, ops):
    return [B.Op(*op) for op in ops]


def iso_start(r):
    """a start on the isokinetic surface m v^2 + Q1 v1^2 / 2 = LkT (tests/test_gpu_thermostats.py)"""
    rng = np.random.default_rng(8)
    kT, Q1 = 2.494, 2.494e-4
    v1 = rng.normal(0, np.sqrt(kT / Q1), (r.n, 3))
    scale = np.sqrt(kT / (r.mass[:, None] * r.v0 ** 2 + 0.5 * Q1 * v1 ** 2))
    return kT, Q1, scale * r.v0, scale * v1


def execute(r, ops, repeat, fuse, start=0, mode=None, resume_entry=False):
    """One run on a fresh context.  Returns the arrays and the counters of the program alone (the first call's are taken off)."""
    B = _backend()
    ctx = B.HipContext(r.n, r.case['box'])
    ctx.set_fuse_inner(fuse)
    for name, value in r.options:
        ctx.set_option(name, value)
    pids = r.define(ctx)
    x, v, m = dev(r.x0), dev(r.v0), dev(r.mass)
    bufs = {s: torch.zeros((r.n, 3), dtype=torch.float64, device='cuda') for s in r.slots}
    ctx.bind_state(x, v, m)
    for s, b in bufs.items():
        ctx.bind_buffer(s, b)
    if mode == 'iso':
        kT, Q1, v_iso, v1 = iso_start(r)
        v.copy_(dev(v_iso))
        bufs[4] = dev(v1)
        ctx.bind_buffer(4, bufs[4])
        ctx.iso_define(True, kT, Q1, 4)
    elif mode == 'regulated':
        ctx.regulated_define(True, 1.0, 2.494)
    if any(op[0] == OP_BATH for op in ops):
        assert ctx.bath_define(float(np.exp(-0.002 * 5.0)), 2.494) == 0
        ctx.expr_seed(424242)
    ctx.run_ops(as_ops(B, r.prologue), 1)
    s0, r0 = ctx.run_stats(), ctx.run_rule_stats()
    if start or resume_entry:
        arr = (B.Op * len(ops))(*as_ops(B, ops))
        cursor = C.c_int64(start)
        if B.lib().amm_run_ops_from(ctx.h, arr, len(ops), int(repeat), C.byref(cursor)) != 0:
            raise B.HipError(B.lib().amm_last_error().decode())
        assert cursor.value == len(ops) * repeat            # (one rank, no exchange: every call runs to the end)
    else:
        ctx.run_ops(as_ops(B, ops), repeat)
    ctx.check()
    s1, r1 = ctx.run_stats(), ctx.run_rule_stats()
    rules = [r1[k] - r0[k] for k in B.RULE_NAMES]
    out = dict(x=x.cpu().numpy().copy(), v=v.cpu().numpy().copy(), bufs={s: b.cpu().numpy().copy() for s, b in bufs.items()},
               builds=[ctx.pair_stats(p)['n_builds'] for p in pids], scheduled=s1['scheduled'] - s0['scheduled'],
               counters=dict(zip(KEYS, rules[:8] + [s1['epilogues'] - s0['epilogues']])))
    assert sum(rules[:7]) == out['scheduled']
    ctx.close()
    return out


WORST = {'x': 0.0, 'v': 0.0}


def total_move(ops, repeat):
    return repeat * sum(abs(op[4]) for op in ops if op[0] == ops_ref.OP_MOVE)


def compare(r, ops, repeat, start=0, mode=None, ref=True, resume_entry=False, label=''):
    """The check of the module docstring; returns the fused and the plain run."""
    fused = execute(r, ops, repeat, True, start, mode, resume_entry)
    plain = execute(r, ops, repeat, False, start, mode, resume_entry)
    print('%s %s: fused %s scheduled %d | plain scheduled %d' % (r.name, label, {k: n for k, n in fused['counters'].items() if n},
                                                                fused['scheduled'], plain['scheduled']))
    assert plain['scheduled'] == len(ops) * repeat - start
    assert plain['counters'] == X(p=plain['scheduled'])
    assert set(fused['bufs']) == set(plain['bufs']) and set(r.slots) <= set(fused['bufs'])
    for name, a, b in [('x', fused['x'], plain['x']), ('v', fused['v'], plain['v'])] + \
                      [('buffer %d' % s, fused['bufs'][s], plain['bufs'][s]) for s in sorted(fused['bufs'])]:
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
        assert np.array_equal(a, b), '%s differs between the fused and the plain run' % name
    assert fused['builds'] == plain['builds']
    if total_move(ops, repeat) > 0 and start < len(ops) * repeat - len(ops) + 1:
        assert np.abs(plain['x'] - r.x0).max() > 1e-4
    if ref and mode is None and r.ref_groups is not None and total_move(ops, repeat) <= REF_HORIZON and \
            all(op[0] in (1, 2, 3, 4, 5) for op in ops):
        want = ops_ref.run(ops, repeat, r.ref_state(), r.ref_groups, start=start)
        dx, dv = np.abs(plain['x'] - want['x']).max(), np.abs(plain['v'] - want['v']).max()
        WORST['x'], WORST['v'] = max(WORST['x'], dx), max(WORST['v'], dv)
        print('    against ops_ref: |dx| %.3e nm, |dv| %.3e nm/ps (worst so far %.3e, %.3e)' % (dx, dv, WORST['x'], WORST['v']))
        assert dx < POS_BOUND and dv < VEL_BOUND
    return fused, plain


# ---------------------------------------------------------------------------------------------------------------- (a) the guards
# kicks: name = buffer(s); coefficients all different, so that a kick moved past another one changes bits
k0, k0b, k0c = K(0, 0.11 * FS), K(0, 0.07 * FS), K(0, 0.05 * FS)
k1, k1b, k1c = K(1, 0.21 * FS), K(1, 0.09 * FS), K(1, 0.04 * FS)
k2, k2b = K(2, 0.34 * FS), K(2, 0.06 * FS)
k3, k3b = K(3, 0.13 * FS), K(3, 0.08 * FS)
k21m, k21p, k31m = K(2, 0.5 * FS, b=1, c=0), K(2, 0.17 * FS, b=1, c=1), K(3, 0.5 * FS, b=1, c=0)
MV = M(0.5 * FS)
H0, D0 = 0.125 * FS, 0.25 * FS
IT0 = [K(0, H0), M(D0), E(0), K(0, H0)]                          # an inner iteration over group 0 (slot 0)
IT0_C2 = [K(0, H0), M(D0), E(0), K(0, 0.1 * FS)]                  # ... whose closing kick has another coefficient
IT0_BATH = [K(0, H0), M(0.5 * D0), (OP_BATH, 0, SLOT_V, 0, 0.0), M(0.5 * D0), E(0), K(0, H0)]
IT3 = [K(1, H0), M(D0), E(3), K(1, H0)]                          # fixture C: an iteration over group 3 (slot 1)
RUN6 = [k2, k3, k21m, k21p, k3b, k1]                              # kick runs (none reads slot 0, the fourth is a two-buffer kick)
PRE7 = [k1, k2, k21m, k21p, k3, k1b, k2b]                         # kicks in front of an inner iteration
TRAIL4 = [k1, k3, k2, k1b]
OPEN3 = [k21m, k3b, k2]


def T(trail):
    """a program that opens with a (two-buffer) KICK and ends in `trail`"""
    return [k21m, MV, E(0)] + trail


def VV(h):
    half = [k1, k3, k1b, k3b, k1c][:h]
    return half + [MV, E(1)] + half


WRAPPED = [k21m, k1] + IT0 + IT0 + [E(2), E(1), k1, k21m]
DUAL_TAIL = [k21m, k1] + IT0 + IT0 + [E(1)]

CASES = []


def case(name, rig_name, ops, repeat, expect, why, declines=(), plan=None):
    CASES.append(dict(id='%s/%s' % (rig_name, name), rig=rig_name, ops=ops, repeat=repeat, expect=expect, why=why, declines=tuple(declines), plan=plan))


# -- kick runs of 1..6 in front of a move: rule 6 takes at most four kicks, the fifth starts a new launch (which takes the move)
for n_ in range(1, 7):
    case('kicks%d-move' % n_, 'W', RUN6[:n_] + [MV, E(0)], 1, X(r6=1 if n_ <= 4 else 2, p=1),
         'rule 6: %s; EVAL(0) plain' % ('the run + MOVE in one launch' if n_ <= 4 else 'four kicks, then the rest + MOVE'))
# -- ... alone (behind them an EVAL): a single kick is no launch of rule 6's (nk == 1 needs the move) and goes plain
for n_ in range(1, 7):
    case('kicks%d-alone' % n_, 'W', [MV, E(1)] + RUN6[:n_] + [E(0)], 1,
         X(p=3 + (1 if n_ in (1, 5) else 0), r6={1: 0, 5: 1, 6: 2}.get(n_, 1)),
         'MOVE, EVAL(1) (no plan: the kicks end the program short of an iteration), EVAL(0) plain; rule 6 takes runs of 2..4, a lone (fifth) kick is plain',
         declines=(6,) if n_ == 1 else ())
# -- ... in front of an inner iteration: rule 2 takes at most three kicks in front of the iteration's own, rule 6 the first four of more
for c_ in range(0, 7):
    case('pre%d-iter' % c_, 'W', PRE7[:c_] + IT0 + [E(1)], 1, X(r2=1, p=1, r6=0 if c_ <= 3 else 1),
         'rule 2: %s; EVAL(1) plain' % ('pre-kicks + iteration in one launch' if c_ <= 3 else 'declines at op 0 (its 4th kick opens no iteration), rule 6 takes four kicks, rule 2 the rest'))
for c_ in range(0, 4):
    case('pre%d-iter3' % c_, 'W', PRE7[:c_] + IT0 * 3 + [E(1)], 1, X(r2=1, p=1), 'rule 2: three equal iterations are one launch')
for c_ in range(0, 4):
    for n_ in (1, 3):
        case('pre%d-bathed%d' % (c_, n_), 'W', PRE7[:c_] + IT0_BATH * n_ + [E(1)], 1, X(r2=1, p=1), 'rule 2: K M BATH M E K iterations are one launch')
case('pre4-bathed1', 'W', PRE7[:4] + IT0_BATH + [E(1)], 1, X(r6=1, r2=1, p=1), 'as pre4-iter: four kicks rule 6, the bathed iteration rule 2')
case('iter-closing-coef', 'W', IT0 + IT0_C2 + IT0 + [E(1)], 1, X(r2=3, p=1),
     'rule 2 compares every iteration with the first of ITS launch: the pattern ends at the odd closing kick, three launches of one iteration')
case('iter-closing-buffer', 'W', [K(0, H0), M(D0), E(0), k1, E(1)], 1, X(r6=1, p=3),
     'closing kick on another buffer: rules 2 and 3 decline; KICK + MOVE rule 6, EVAL(0), the kick, EVAL(1) plain', declines=(2, 3))
# -- trailing blocks of a program that opens with a KICK: rule 1 defers at most three kicks, in every repetition but the last; the next
#    repetition's opening launch (rule 6: deferred + own kicks <= 4, + MOVE) takes them along
for t_ in range(1, 5):
    for r_ in (1, 2, 3):
        if t_ == 4:
            exp_, why_ = X(r6=2 * r_, p=r_), 'four trailing kicks: rule 1 declines (nk > 3); per repetition KICK + MOVE (6), EVAL (plain), four kicks (6)'
        else:
            last = X(p=1) if t_ == 1 else X(r6=1)              # the last repetition's trailing kicks: nothing to defer into
            exp_ = X(r1=r_ - 1, r6=r_ + last['r6'], p=r_ + last['p'])
            why_ = 'per repetition: opening launch (6, with the deferred kicks), EVAL (plain), trailing kicks: rule 1 but in the last repetition (%s)' % ('plain' if t_ == 1 else 'rule 6')
        case('trail%d-r%d' % (t_, r_), 'W', T(TRAIL4[:t_]), r_, exp_, why_, declines=(1,) if (t_ == 4 or r_ == 1) else ())
case('trail-copy-safe-r2', 'W', T([k1, CP(3, 2), k3]), 2, X(r1=1, r6=2, p=5),
     'COPY(3 <- 2): no earlier kick of the block reads slot 3 -> deferred (copy runs now); EVAL(0) plain twice; last repetition: K, COPY, K plain')
case('trail-copy-safe-r3', 'W', T([k1, CP(3, 2), k3]), 3, X(r1=2, r6=3, p=6), 'as r2, one more deferring repetition: EVAL(0) three times + K, COPY, K')
case('trail-copy-dest-read-r2', 'W', T([k3, CP(3, 2)]), 2, X(r6=2, p=6),
     'COPY(3 <- 2) behind a kick that reads slot 3: rule 1 declines; per repetition K + M (6), EVAL, kick, COPY plain', declines=(1,))
case('trail-copy-dest-read-r3', 'W', T([k3, CP(3, 2)]), 3, X(r6=3, p=9), 'as r2', declines=(1,))
case('trail-copy-slot-v-r2', 'W', T([k1, CP(3, SLOT_V)]), 2, X(r6=2, p=6), 'a COPY that touches SLOT_V: rule 1 declines', declines=(1,))
# -- deferred kicks met by each taker
case('defer-meets-rule2-r2', 'W', IT0 + [k1, k3], 2, X(r2=2, r1=1, r6=1), 'rule 2 leads its launch with the two deferred kicks; last repetition: two kicks rule 6')
case('defer-meets-rule2-r3', 'W', IT0 + [k1, k3], 3, X(r2=3, r1=2, r6=1), 'as r2')
case('defer-meets-rule3-guard-r2', 'W', [k2, MV, E(0), k1, k3], 2, X(r1=1, r6=3, p=2),
     'op 0 is K ; M ; E with a closing kick on another buffer: rule 3 flushes the deferred kicks, then declines; K + M rule 6', declines=(2, 3))
for d_, u_ in ((3, 1), (2, 2), (3, 2), (2, 3)):
    case('defer%d-run%d-r2' % (d_, u_), 'W', OPEN3[:u_] + [MV, E(0)] + TRAIL4[:d_], 2, X(r1=1, r6=3, p=2),
         'ndef + run = %d: %s; counters alike: opening launch (6), EVAL, rule 1 / opening launch (6), EVAL, trailing kicks (6)'
         % (d_ + u_, 'rule 6 takes the deferred kicks along' if d_ + u_ <= 4 else 'rule 2 flushes them (more than four), rule 6 takes its own'))
# -- rule 4 and the molecule-row plans
case('dual-E2E1-plan', 'W', [E(2), E(1)] + DUAL_TAIL, 1, X(r4=1, off=1, epi=1, p=1), 'one pass for both, its launch carries 2 pre-kicks + 2 iterations; EVAL(1) plain', plan='mol')
case('dual-E1E2-plan', 'W', [E(1), E(2)] + DUAL_TAIL, 1, X(r4=1, off=1, epi=1, p=1), 'the order of the two EVALs is free', plan='mol')
case('dual-copy', 'W', [E(2), E(1), CP(3, 2), k31m, k1] + IT0 + IT0 + [E(1)], 1, X(r4=1, p=2, r2=1),
     'a COPY behind the EVALs: no plan (no kick at once), shared pass still; COPY plain, kicks + iterations rule 2, EVAL plain', plan='mol')
case('dual-pre6', 'W', [E(2), E(1)] + PRE7[:6] + IT0 + [E(1)], 1, X(r4=1, off=1, epi=1, p=1), 'six pre-kicks = AMM_MAX_PRE: planned and carried', plan='mol')
case('dual-pre7', 'W', [E(2), E(1)] + PRE7 + IT0 + [E(1)], 1, X(r4=1, r6=1, r2=1, p=1),
     'seven pre-kicks: kick_run stops at 7, the 7th is followed by a KICK, not a MOVE: no plan; four kicks rule 6, three + iteration rule 2', plan='mol')
case('unshared-E2E1-plan', 'W-unshared', [E(2), E(1)] + DUAL_TAIL, 1, X(p=3, off=1, epi=1),
     'lists of their own: rule 4 declines; EVAL(2) plain, EVAL(1) plain with the plan on its own launch, EVAL(1) plain', declines=(4,), plan='mol')
case('nositetab-E2E1-plan', 'W-nositetab', [E(2), E(1)] + DUAL_TAIL, 1, X(r4=1, off=1, r2=1, p=1),
     'no site tables: the plan is offered, no kernel carries it; kicks + iterations rule 2', plan='mol')
case('wrapped-r1', 'W', WRAPPED, 1, X(r2=1, r4=1, r6=1), 'one repetition: nothing to wrap into, the closing kicks are rule 6', plan='mol')
case('wrapped-r2', 'W', WRAPPED, 2, X(r2=1, r4=2, r6=1, off=1, epi=1),
     'the first shared pass carries the closing kicks, the opening kicks and both iterations of repetition 2, which starts at its EVALs', plan='mol')
case('wrapped-r3', 'W', WRAPPED, 3, X(r2=1, r4=3, r6=1, off=2, epi=2), 'as r2, twice', plan='mol')
# -- per-atom plans: a velocity-Verlet program with h kicks per half step
case('vv1-r1', 'L', VV(1), 1, X(r6=1, p=2), 'K + M rule 6; the last step closing kick is not planned (nothing follows): EVAL, kick plain', plan='atom')
case('vv1-r3', 'L', VV(1), 3, X(r6=1, p=4, off=2, epi=2), 'EVALs 1 and 2 carry closing kick + opening kick + MOVE (the next repetition starts at its EVAL); the third and the last kick plain', plan='atom')
case('vv2-r3', 'L', VV(2), 3, X(r6=2, p=3, off=2, epi=2), 'four kicks on a plan; opening 2 K + M and closing 2 K rule 6', plan='atom')
case('vv4-r1', 'L', VV(4), 1, X(r6=2, p=1), 'no plan in the last repetition', plan='atom')
case('vv4-r3', 'L', VV(4), 3, X(r6=6, p=3), 'closing + opening kicks are eight: the fifth kick declines the plan; rule 1 declines four trailing kicks', declines=(1,), plan='atom')
case('vv5-r1', 'L', VV(5), 1, X(r6=3, p=2), '4 K, K + M, EVAL, 4 K, lone kick plain', plan='atom')
case('vv5-r3', 'L', VV(5), 3, X(r6=9, r1=2, p=4), 'per repetition 4 K, K + M, EVAL, 4 K; the lone fifth trailing kick is deferred (rule 1), flushed by rule 2 (1 + 5 > 4); plain in the end', plan='atom')
case('vv1-r3-no-kernel', 'L-nochargeless', VV(1), 3, X(r6=3, r1=2, p=4, off=2),
     'option chargeless = 0: plans offered, no kernel carries them: the closing kick is deferred (rule 1), flushed by rule 3 guard, K + M rule 6', plan='atom')
# -- rule 3 (components above 8 atoms: rule 2 declines), the ping-pong, f0_slot
for n_ in (1, 2, 3):
    case('iter%d' % n_, 'C', IT0 * n_ + [E(3)], 1, X(r3=n_, p=1), 'one launch per iteration (odd counts: state copied back at the end)', declines=(2,))
case('odd-then-ops', 'C', IT0 + [CP(3, 0), CB(3, 0, 0.5, 3), k3, CP(3, SLOT_X), k3b, k1, E(3)] + IT3 + [E(0)], 1, X(r3=1, p=8, r6=2),
     'swapped: COPY, COMBINE, kick, COPY(<- SLOT_X) plain, 2 kicks rule 6, EVAL(3) plain, iteration over group 3 declined (f0_slot taken): K + M rule 6, EVAL, kick, EVAL plain')
case('even-then-group3', 'C', IT0 * 2 + IT3 + [E(0)], 1, X(r3=2, r6=1, p=3), 'not swapped, f0_slot = 0: the iteration over group 3 goes K + M (6), EVAL, kick plain')
case('group3-first', 'C', IT3 + IT0 + [E(0)], 1, X(r3=1, r6=1, p=3), 'f0_slot = 1 is taken by group 3: the iteration over group 0 goes plain')
case('trailing-after-iter-r2', 'C', IT0 + [k1, k3], 2, X(r3=2, r6=2), 'rule 1 declines behind rule 3 (swapped / f0_slot): the trailing kicks are rule 6 in both repetitions', declines=(1,))
case('EKKM-not-term-parallel', 'C', [E(0), k0, k1, MV, E(3)], 1, X(p=2, r6=1), 'terms_from above the set: rule 5 declines', declines=(5,))
# -- rule 5
for rig_, g2_, ka_, kb_ in (('C5', 3, k1, k1b), ('H', 0, k3, k3b)):
    case('EK', rig_, [MV, E(0), k0, E(g2_), MV], 1, X(r5=1, p=3), 'EVAL + kick one launch; MOVE, EVAL, MOVE plain')
    case('EKKM', rig_, [E(0), k0, ka_, MV, E(g2_)], 1, X(r5=1, p=1), 'EVAL + 2 kicks + MOVE one launch')
    case('E5K', rig_, [MV, E(0), k0, ka_, k0b, kb_, k0c, E(g2_)], 1, X(r5=1, p=3), 'EVAL + four kicks; the fifth kick plain (alone)')
    case('EKMM', rig_, [E(0), k0, MV, MV, E(g2_)], 1, X(r5=1, p=2), 'the second MOVE is plain')

BY_ID = {c_['id']: c_ for c_ in CASES}
OBSERVED = {}


def run_case(c_):
    fused, _ = compare(rig(c_['rig']), c_['ops'], c_['repeat'], label=c_['id'])
    OBSERVED[c_['id']] = fused['counters']
    return fused['counters']


@pytest.mark.parametrize('cid', [c_['id'] for c_ in CASES])
def test_programs_on_the_guards(cid):
    c_ = BY_ID[cid]
    got = run_case(c_)
    assert got == c_['expect'], '%s: derived %s (%s), the scheduler did %s' % (cid, {k: n for k, n in c_['expect'].items() if n}, c_['why'],
                                                                             {k: n for k, n in got.items() if n})


def test_every_rule_and_plan_fires_and_declines_somewhere():
    """Over the counters the cases above collected (a case not run yet is run here): each of rules 1..6 has a case where it fires and a
    case whose program sits on its guard and where it stays at 0; both kinds of plan have a carried and a declined case."""
    seen = {c_['id']: OBSERVED.get(c_['id']) or run_case(c_) for c_ in CASES}
    for rule in range(1, 7):
        key = 'r%d' % rule
        assert any(s[key] > 0 for s in seen.values()), 'rule %d never fires' % rule
        assert any(rule in c_['declines'] and seen[c_['id']][key] == 0 for c_ in CASES), 'no case where rule %d declines' % rule
    for kind in ('mol', 'atom'):
        mine = [seen[c_['id']] for c_ in CASES if c_['plan'] == kind]
        assert any(s['epi'] > 0 for s in mine), 'no carried %s plan' % kind
        assert any(s['epi'] == 0 for s in mine), 'no declined %s plan' % kind
        assert any(s['epi'] == 0 and s['off'] > 0 for s in mine), 'no %s plan that was offered and not carried' % kind


# ---------------------------------------------------------------------------------------------------------------- (b) random programs
def random_program(name, seed):
    """3..8 blocks; every MOVE of a repetition shares 2 fs, every kick coefficient is at most 0.25 fs (far below the 2 fs allowed: a
    program may kick many times with forces it never evaluates again)."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    slots = {'W': (0, 1, 2, 3), 'C': (0, 1, 3), 'L': (1, 2, 3)}[name]
    groups = {'W': (0, 1, 2), 'C': (0, 3), 'L': (1, 2)}[name]
    g_it, s_it = {'W': (0, 0), 'C': (0, 0), 'L': (1, 1)}[name]

    def kick():
        coef = float(rng.uniform(0.02, 0.25) * FS * rng.choice([-1.0, 1.0]))
        if rng.integers(3) == 0:
            a, b = rng.choice(slots, 2, replace=False)
            return K(int(a), coef, b=int(b), c=int(rng.integers(2)))
        return K(int(rng.choice(slots)), coef)

    blocks = []
    for _ in range(int(rng.integers(3, 9))):
        kind = int(rng.integers(7))
        if kind == 0:
            blocks.append([kick() for _ in range(int(rng.integers(1, 7)))])
        elif kind == 1:
            blocks.append([M(1.0)])
        elif kind == 2:
            blocks.append([E(int(rng.choice(groups)))])
        elif kind == 3:
            a, b = rng.choice(groups, 2, replace=False)
            blocks.append([E(int(a)), E(int(b))])
        elif kind == 4:
            h, h2 = float(rng.uniform(0.02, 0.25) * FS), float(rng.uniform(0.02, 0.25) * FS)
            blocks.append([K(s_it, h), M(1.0), E(g_it), K(s_it, h2 if rng.integers(2) else h)] * int(rng.integers(1, 5)))
        elif kind == 5:
            blocks.append([CP(3, int(rng.choice([s for s in slots if s != 3])))])
        else:
            s, t = rng.choice(slots, 2)
            blocks.append([CB(3, int(s), float(rng.uniform(-1.0, 1.0)), int(t))])
    ops = [op for b in blocks for op in b]
    adjacent = any(ops[i][0] == 2 and ops[i + 1][0] in (2, 3) for i in range(len(ops) - 1))
    if not adjacent:
        ops += [kick(), M(1.0)]
    moves = [i for i, op in enumerate(ops) if op[0] == 3]
    if not moves:
        ops += [kick(), M(1.0)]
        moves = [len(ops) - 1]
    share = rng.uniform(0.5, 1.0, len(moves))
    share = share / share.sum() * rng.uniform(1.0, 2.0) * FS
    for i, d in zip(moves, share):
        ops[i] = M(float(d))
    return ops, int(rng.integers(1, 4))


@pytest.mark.parametrize('seed', range(24))
@pytest.mark.parametrize('name', ['W', 'C', 'L'])
def test_structured_random_programs(name, seed):
    ops, repeat = random_program(name, seed)
    assert any(ops[i][0] == 2 and ops[i + 1][0] in (2, 3) for i in range(len(ops) - 1))
    assert total_move(ops, 1) <= 2 * FS + 1e-15 and max(abs(op[4]) for op in ops if op[0] == 2) <= 2 * FS
    fused, plain = compare(rig(name), ops, repeat, ref=name in ('W', 'L') and seed < 8, label='random %d (%d ops x %d)' % (seed, len(ops), repeat))
    # an adjacent KICK, KICK or KICK, MOVE is one launch under every rule that can meet it: fewer decisions than ops, always
    assert fused['scheduled'] < plain['scheduled']


# ---------------------------------------------------------------------------------------------------------------- (c) resumption
RESUMED = [('W', 'rule 1', T(TRAIL4[:2]), 2), ('W', 'rule 2', PRE7[:2] + IT0 * 2 + [E(1)], 2), ('C', 'rule 3', IT0 * 3 + [E(3)], 2),
           ('W', 'rule 4 + wrapped plan', WRAPPED, 2), ('C5', 'rule 5', [E(0), k0, k1, MV, E(3)], 2), ('L', 'rule 6 + per-atom plan', VV(2), 3)]


@pytest.mark.parametrize('which', range(len(RESUMED)), ids=[r_[1].replace(' ', '-') for r_ in RESUMED])
def test_resumption_at_every_cursor(which):
    """amm_run_ops_from started at every unrolled index of the first two repetitions (one rank, no exchange: each call runs to the end):
    bit for bit the plain context started at the same cursor, and the reference interpreter started there."""
    name, label, ops, repeat = RESUMED[which]
    for start in range(0, 2 * len(ops)):
        compare(rig(name), ops, repeat, start=start, resume_entry=True, label='%s from %d' % (label, start))


# ---------------------------------------------------------------------------------------------------------------- (d) modes
MODE_PROGRAMS = [('kicks5-move', RUN6[:5] + [MV, E(0)], 1), ('pre2-iter3', PRE7[:2] + IT0 * 3 + [E(1)], 1),
                 ('dual-E2E1-plan', [E(2), E(1)] + DUAL_TAIL, 1), ('trail2-r2', T(TRAIL4[:2]), 2)]


@pytest.mark.parametrize('mode', ['iso', 'regulated'])
def test_modes_keep_their_rules_off(mode):
    """Isokinetic mode (every KICK rescales v and v1): rules 3, 5, 6 and both plans stay off.  Regulated mode (every MOVE is the regulated
    one): rules 3, 5 and the plans stay off, rule 6 -- whose launch knows the mode -- fires.  Fused == plain bit for bit, v1 included."""
    r = rig('W')
    r6 = 0
    for label, ops, repeat in MODE_PROGRAMS:
        fused, _ = compare(r, ops, repeat, mode=mode, label='%s %s' % (mode, label))
        got = fused['counters']
        assert got['r3'] == 0 and got['r5'] == 0 and got['off'] == 0 and got['epi'] == 0, got
        if mode == 'iso':
            assert got['r6'] == 0 and 4 in fused['bufs'], got
        r6 += got['r6']
        if label == 'dual-E2E1-plan':
            assert got['r4'] == 1          # (the shared pass itself knows no mode)
        if label == 'pre2-iter3':
            assert got['r2'] == 1          # (the component-parallel loop knows both modes)
    assert (r6 > 0) == (mode == 'regulated')
