"""CPU tests of tests/ops_ref.py, the reference interpreter that tests/test_gpu_op_programs.py holds amm_run_ops against.

1. Fed the RESPA [4, 2, 1] op list of test_respa_ops_vs_oracle_trajectory it gives, bit for bit, what that test's loops over the oracle
   give (both take the list and the loops from ops_ref).
2. On a six-atom toy state with a closed-form force every op kind, `repeat` and `start` are compared with a machine that evaluates each op
   with mpmath at 50 digits from the doubles in front of it and rounds the result ONCE.  The interpreter rounds a kick three times
   (coef * f, / m, v +), a MOVE and a COMBINE twice.  The roundings it adds sit on the increment; in every kick and move here that is
   scaled by |coef| / m <= 2^-8 against the value it is added to, and the COMBINEs either multiply by -1 (exact) or add a product that is
   smaller than their result, so an op's result is the correctly rounded one or its neighbour: 1 ulp, as the comparison asks.
"""
import mpmath
import numpy as np
import pytest

import ops_ref
from ops_ref import CB, CP, E, K, M, SLOT_V, SLOT_X
from oracle import oracle as O

mpmath.mp.dps = 50
N = 6
CENTRE = np.array([[0.11, -0.23, 0.31], [0.47, 0.05, -0.38], [-0.52, 0.29, 0.17], [0.08, 0.61, -0.44], [-0.33, -0.12, 0.56], [0.24, -0.49, -0.07]])
STIFF = np.array([310.0, 470.5, 123.25, 288.0, 95.75, 512.5])


def toy_force(scale):
    """f = -scale k (x - c) + scale sin(3 x): evaluated at 50 digits and rounded once, so that both machines see the same doubles"""
    def f(x):
        out = np.empty_like(x)
        for i in range(N):
            for d in range(3):
                xv = mpmath.mpf(float(x[i, d]))
                out[i, d] = float(-scale * mpmath.mpf(float(STIFF[i])) * (xv - mpmath.mpf(float(CENTRE[i, d]))) + scale * mpmath.sin(3 * xv))
        return out
    return f


GROUPS = {0: (0, [toy_force(1.0)]), 1: (1, [toy_force(0.375)]), 2: (2, [toy_force(0.0625), toy_force(-0.21875)])}


def toy_state():
    rng = np.random.default_rng(20250101)
    x = CENTRE + rng.normal(scale=0.02, size=(N, 3))
    v = rng.normal(scale=0.6, size=(N, 3))
    mass = np.array([15.999, 1.008, 1.008, 12.011, 14.007, 32.06])
    return ops_ref.new_state(x, v, mass, range(4))


def mp_machine(ops, repeat, state, start=0):
    """Every op at 50 digits from the doubles it finds, its result rounded to double once."""
    x, v, m, bufs = state['x'], state['v'], state['mass'], state['bufs']
    mpf = lambda a: mpmath.mpf(float(a))                                    # noqa: E731

    def buf(s):
        return x if s == SLOT_X else v if s == SLOT_V else bufs[s]

    for at in range(start, repeat * len(ops)):
        op, a, b, c, coef = ops[at % len(ops)]
        if op == ops_ref.OP_EVAL:
            slot, members = GROUPS[a]
            fs = [member(x) for member in members]
            buf(slot)[...] = [[float(sum(mpf(f[i, d]) for f in fs)) for d in range(3)] for i in range(N)]
        elif op == ops_ref.OP_KICK:
            fa, fb = buf(a), (buf(b) if b >= 0 else None)
            for i in range(N):
                for d in range(3):
                    ff = mpf(fa[i, d]) if fb is None else (mpf(fa[i, d]) + mpf(fb[i, d]) if c else mpf(fa[i, d]) - mpf(fb[i, d]))
                    v[i, d] = float(mpf(v[i, d]) + mpf(coef) * ff / mpf(m[i]))
        elif op == ops_ref.OP_MOVE:
            for i in range(N):
                for d in range(3):
                    x[i, d] = float(mpf(x[i, d]) + mpf(coef) * mpf(v[i, d]))
        elif op == ops_ref.OP_COPY:
            buf(a)[...] = buf(b)
        elif op == ops_ref.OP_COMBINE:
            sa, sb = buf(b).copy(), buf(c).copy()
            buf(a)[...] = [[float(mpf(sa[i, d]) + mpf(coef) * mpf(sb[i, d])) for d in range(3)] for i in range(N)]
        else:
            raise AssertionError(op)
    return state


def arrays(state):
    return [('x', state['x']), ('v', state['v'])] + [('buf%d' % s, state['bufs'][s]) for s in sorted(state['bufs'])]


def assert_within_one_ulp(got, ref):
    for (name, a), (_, b) in zip(arrays(got), arrays(ref)):
        assert np.isfinite(a).all()
        ulps = np.abs(a - b) / np.spacing(np.abs(b))
        assert ulps.max() <= 1.0, (name, ulps.max())


DT = 0.002
PROLOGUE = [E(0), E(1), E(2)]
STEP = [K(2, 0.5 * DT, b=1), K(0, 0.25 * DT), M(0.5 * DT), E(0), K(0, 0.25 * DT), CP(3, 1), E(1), CB(3, 2, -1.0, 3), K(3, 0.5 * DT, b=1, c=1), E(2)]
CASES = {
    'kick-single': (PROLOGUE + [K(0, DT)], 1, 0),
    'kick-minus': (PROLOGUE + [K(2, DT, b=1, c=0)], 1, 0),
    'kick-plus': (PROLOGUE + [K(2, DT, b=1, c=1)], 1, 0),
    'move': ([M(DT)], 1, 0),
    'copy-to-slot-v': (PROLOGUE + [CP(SLOT_V, 1), M(1e-6)], 1, 0),
    'copy-from-slot-v': ([CP(3, SLOT_V), CP(2, SLOT_X), K(3, DT, b=2, c=1)], 1, 0),
    'combine': (PROLOGUE + [CB(3, 0, -0.4375, 1), CB(3, 3, 0.3, 3), K(3, DT)], 1, 0),
    'repeat-3': (PROLOGUE + STEP, 3, 0),
    'start-in-the-middle': (PROLOGUE + STEP, 3, len(PROLOGUE + STEP) + 5),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_op_kind_against_mpmath(name):
    ops, repeat, start = CASES[name]
    warm = [] if ops[:3] == PROLOGUE and start == 0 else PROLOGUE          # (programs that do not evaluate first: the buffers hold forces)
    got, ref = toy_state(), toy_state()
    for state in (got, ref):
        mp_machine(warm, 1, state)
    before = [a.copy() for _, a in arrays(got)]
    assert ops_ref.run(ops, repeat, got, GROUPS, start=start) is got
    mp_machine(ops, repeat, ref, start=start)
    assert_within_one_ulp(got, ref)
    changed = [not np.array_equal(a, b) for (_, a), b in zip(arrays(got), before)]
    assert any(changed[:2])                                                 # every case moves x or v


def test_start_composes_with_single_ops():
    """run(start = i) == the op at i on its own, then run(start = i + 1): the cursor is the unrolled index, nothing else is carried"""
    ops, repeat = PROLOGUE + STEP, 2
    for start in range(0, repeat * len(ops) + 1):
        whole, parts = toy_state(), toy_state()
        ops_ref.run(ops, repeat, whole, GROUPS, start=start)
        if start < repeat * len(ops):
            ops_ref.run([ops[start % len(ops)]], 1, parts, GROUPS)
            ops_ref.run(ops, repeat, parts, GROUPS, start=start + 1)
        for (name, a), (_, b) in zip(arrays(whole), arrays(parts)):
            assert np.array_equal(a, b), (start, name)
    with pytest.raises(ValueError):
        ops_ref.run(ops, repeat, toy_state(), GROUPS, start=repeat * len(ops) + 1)


@pytest.mark.parametrize('op', [6, 7, 8, 9, 10, 11, 12, 99])
def test_ops_out_of_scope_raise(op):
    with pytest.raises(NotImplementedError):
        ops_ref.run([(op, 0, 0, 0, 0.0)], 1, toy_state(), GROUPS)


def test_unbound_buffer_raises():
    with pytest.raises(KeyError):
        ops_ref.run([K(7, DT)], 1, toy_state(), GROUPS)


def test_accepts_backend_ops():
    from atomsmm_amd import backend as B
    a, b = toy_state(), toy_state()
    ops_ref.run(PROLOGUE + STEP, 2, a, GROUPS)
    ops_ref.run([B.Op(*op) for op in PROLOGUE + STEP], 2, b, GROUPS)
    for (name, p), (_, q) in zip(arrays(a), arrays(b)):
        assert np.array_equal(p, q), name
    assert (B.OP_EVAL, B.OP_KICK, B.OP_MOVE, B.OP_COPY, B.OP_COMBINE, B.SLOT_X, B.SLOT_V) == \
        (ops_ref.OP_EVAL, ops_ref.OP_KICK, ops_ref.OP_MOVE, ops_ref.OP_COPY, ops_ref.OP_COMBINE, SLOT_X, SLOT_V)


def test_respa_program_equals_the_hand_written_oracle_loop(spcfw):
    """The op list and the state of test_respa_ops_vs_oracle_trajectory (tests/test_gpu_abi_parity.py)."""
    c = spcfw
    n = len(c['positions'])
    dt = 0.004
    rng = np.random.default_rng(11)
    x = c['positions'].copy()
    m = c['mass'].copy()
    v = rng.normal(size=(n, 3)) * np.sqrt(2.494 / m)[:, None]
    dn = O.desc(O.ADJ['force-switch'], rc=0.7, rc0=0.7, rs0=0.5)
    dd = O.desc(O.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1)

    def f0(p):
        return (O.harmonic_bonds(c['bonds'], c['bond_r0'], c['bond_k'], p, c['box'])[1] +
                O.harmonic_angles(c['angles'], c['angle_theta0'], c['angle_k'], p, c['box'])[1])

    def f1(p):
        return O.pair_eval(dn, p, c['box'], c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'])[1]

    def f2(p):
        return O.pair_eval(dd, p, c['box'], c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'])[1]

    xo, vo = ops_ref.respa_421_by_hand(f0, f1, f2, x, v, m, dt, 2)
    groups = {0: (0, ops_ref.oracle_forces(c, bonds=True, angles=True)), 1: (1, ops_ref.oracle_forces(c, pair=dn)),
              2: (2, ops_ref.oracle_forces(c, pair=dd))}
    state = ops_ref.run(ops_ref.respa_421_ops(dt), 2, ops_ref.new_state(x, v, m, range(4)), groups)
    assert np.array_equal(state['x'], xo) and np.array_equal(state['v'], vo)
    assert np.abs(xo - x).max() > 1e-3
    # the buffers at the end of the program: the forces of the last evaluations, and the scratch copy of f2
    assert np.array_equal(state['bufs'][2], f2(xo)) and np.array_equal(state['bufs'][3], state['bufs'][2])
    assert np.array_equal(state['bufs'][0], f0(xo)) and np.array_equal(state['bufs'][1], f1(xo))
