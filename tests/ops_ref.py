"""Reference interpreter of amm_run_ops step programs (test infrastructure; CPU: numpy + the C oracle).

run() walks the flat op list exactly as include/atomsmm_hip.h defines the ops, one op after the other and nothing else: no fusion,
no deferral, no second set of buffers.  It is what the scheduler in csrc/run_ops.hip must reproduce whatever it fuses.

    EVAL g       buf[slot(g)] <- sum of the group's forces at the current x (callables; oracle_forces() builds them from oracle.oracle)
    KICK a b c   v <- v + (coef * (buf[a] -/+ buf[b])) / m      (b = -1: buf[a] alone; c = 1: plus) -- oracle.kick, its rounding order
    MOVE         x <- x + coef * v                                                                   -- oracle.move
    COPY a b     buf[a] <- buf[b]
    COMBINE      buf[a] <- buf[b] + coef * buf[c]
SLOT_X / SLOT_V are the state itself.  BATH, EXPR, STOCK, the constraint ops, ALLREDUCE and the isokinetic / regulated modes are not
restated here: run() raises on them.
"""
import numpy as np

from oracle import oracle as O

OP_EVAL, OP_KICK, OP_MOVE, OP_COPY, OP_COMBINE = 1, 2, 3, 4, 5
SLOT_X, SLOT_V = 62, 63
OP_NAMES = {6: 'EXPR', 7: 'BATH', 8: 'SAVE_REF', 9: 'CONSTRAIN_X', 10: 'CONSTRAIN_V', 11: 'ALLREDUCE', 12: 'STOCK'}


def E(g):
    return (OP_EVAL, g, 0, 0, 0.0)


def K(a, coef, b=-1, c=0):
    return (OP_KICK, a, b, c, float(coef))


def M(coef):
    return (OP_MOVE, 0, 0, 0, float(coef))


def CP(dst, src):
    return (OP_COPY, dst, src, 0, 0.0)


def CB(dst, a, coef, b):
    """buf[dst] <- buf[a] + coef * buf[b]"""
    return (OP_COMBINE, dst, a, b, float(coef))


def fields(op):
    """(op, a, b, c, coef) of a tuple or of a backend.Op"""
    return (op.op, op.a, op.b, op.c, op.coef) if hasattr(op, 'coef') else tuple(op)


def respa_421_ops(dt):
    """One outer step of RespaPropagator([4, 2, 1]) over groups 0 (slot 0), 1 (slot 1), 2 (slot 2) with slot 3 as scratch, as
    tests/test_gpu_abi_parity.py::test_respa_ops_vs_oracle_trajectory runs it."""
    ops = [E(2), E(1), CP(3, 2), K(3, 0.5 * dt, b=1)]
    for _n1 in range(2):
        ops += [K(1, 0.25 * dt), E(0)]
        for _n0 in range(4):
            ops += [K(0, 0.0625 * dt), M(0.125 * dt), E(0), K(0, 0.0625 * dt)]
        ops += [E(1), K(1, 0.25 * dt)]
    ops += [E(2), CP(3, 2), K(3, 0.5 * dt, b=1)]
    return ops


def respa_421_by_hand(f0, f1, f2, x, v, m, dt, nsteps):
    """The same program written out as loops over the oracle (the exact op order of SURVEY.md 3.2), not as an op list: what
    test_respa_ops_vs_oracle_trajectory compares the GPU with, and what run(respa_421_ops(dt), nsteps, ...) must give bit for bit.
    f0, f1, f2: x -> forces of the three groups.  Returns the final (x, v)."""
    xo, vo = x.copy(), v.copy()
    for _ in range(nsteps):
        F2 = f2(xo); F1 = f1(xo)
        O.kick(vo, F2, m, 0.5 * dt, fsub=F1)
        for _n1 in range(2):
            O.kick(vo, F1, m, 0.25 * dt)
            F0 = f0(xo)
            for _n0 in range(4):
                O.kick(vo, F0, m, 0.0625 * dt)
                O.move(xo, vo, 0.125 * dt)
                F0 = f0(xo)
                O.kick(vo, F0, m, 0.0625 * dt)
            F1 = f1(xo)
            O.kick(vo, F1, m, 0.25 * dt)
        F2 = f2(xo)
        O.kick(vo, F2, m, 0.5 * dt, fsub=F1)
    return xo, vo


def oracle_forces(case, bonds=False, angles=False, torsions=False, pair=None, periodic=False):
    """Callables x -> forces [n][3] over oracle.oracle for the arrays of a test case (tests/golden/*.npz, atomsmm_amd.testing): the
    members a group is made of.  pair: an oracle.desc; periodic: the bond-list terms take the nearest image."""
    box = case['box']
    out = []
    if bonds:
        out.append(lambda x: O.harmonic_bonds(case['bonds'], case['bond_r0'], case['bond_k'], x, box, periodic)[1])
    if angles:
        out.append(lambda x: O.harmonic_angles(case['angles'], case['angle_theta0'], case['angle_k'], x, box, periodic)[1])
    if torsions:
        out.append(lambda x: O.periodic_torsions(case['torsions'], case['torsion_n'], case['torsion_phase'], case['torsion_k'], x, box, periodic)[1])
    if pair is not None:
        excl = case.get('exc_pairs')
        csr = O.exclusion_csr(len(case['charge']), excl) if excl is not None and len(excl) else None
        out.append(lambda x: O.pair_eval(pair, x, box, case['charge'], case['sigma'], case['epsilon'], None, csr=csr)[1])
    return out


def new_state(x, v, mass, slots):
    """x, v [n][3], mass [n]; the bound buffers `slots` start at zero"""
    x = np.array(x, dtype=np.float64, order='C')
    return dict(x=x, v=np.array(v, dtype=np.float64, order='C'), mass=np.array(mass, dtype=np.float64),
                bufs={int(s): np.zeros_like(x) for s in slots})


def run(ops, repeat, state, groups, start=0):
    """Interpret `ops`, `repeat` times over, from the unrolled index `start` = rep * n_ops + k (amm_run_ops_from's cursor).
    state: new_state(); changed in place and returned.  groups: {group: (slot, [callable x -> forces, ...])}."""
    ops = [fields(o) for o in ops]
    n_ops = len(ops)
    if not 0 <= start <= repeat * n_ops:
        raise ValueError('start out of range')
    x, v, m, bufs = state['x'], state['v'], state['mass'], state['bufs']

    def buf(s):
        if s == SLOT_X:
            return x
        if s == SLOT_V:
            return v
        if s not in bufs:
            raise KeyError('buffer slot %d is not bound' % s)
        return bufs[s]

    for at in range(start, repeat * n_ops):
        op, a, b, c, coef = ops[at % n_ops]
        if op == OP_EVAL:
            slot, members = groups[a]
            total = np.zeros_like(x)
            for q, member in enumerate(members):
                f = np.asarray(member(x), dtype=np.float64)
                total = f.copy() if q == 0 else total + f
            buf(slot)[...] = total
        elif op == OP_KICK:
            if b < 0:
                O.kick(v, buf(a), m, coef)
            else:
                # oracle.kick subtracts: a plus kick hands it the negated buffer (fa - (-fb) is fa + fb, bit for bit)
                O.kick(v, buf(a), m, coef, fsub=-buf(b) if c else buf(b))
        elif op == OP_MOVE:
            O.move(x, v, coef)
        elif op == OP_COPY:
            buf(a)[...] = buf(b)
        elif op == OP_COMBINE:
            buf(a)[...] = buf(b) + coef * buf(c)
        else:
            raise NotImplementedError('ops_ref.run does not restate op %s' % OP_NAMES.get(op, op))
    return state
