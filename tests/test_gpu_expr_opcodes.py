"""Both expression interpreters of csrc/expr.hip, opcode by opcode, through the C ABI (amm_expr_eval: k_expr / expr_run;
amm_expr_eval_scalar: k_expr_scalar) against the mpmath evaluator of tests/expr_reference.py -- which reads the TEXT, so the compiler
of atomsmm_amd/expr.py is under test with them -- and the random stream against the Philox-4x32-10 of oracle/expr_oracle.py, which
tests/test_expr_semantics_host.py anchors to the published known-answer vectors.

Shapes: 1, 21, 22 and 86 atoms = 3, 63, 66, 258 degrees of freedom (below one wavefront, across one, one 256-thread block plus two
lanes); the opcode tables run at 86 with their inputs cycled.

Bounds.  + - * /, negation, abs, floor, ceil, step, delta, min, max, select: the correctly rounded value (mpmath has no signed zero:
+0 and -0 count as equal).  x^n with a literal n: relative error |n| 2^-52 (one rounding per multiplication).  sqrt, the
transcendentals, pow, atan2: no accuracy statement of the device library is known to this project, so MEASURED_ULP holds the largest
error against mpmath that an MI355X gave on the fixed inputs of expr_reference.TABLE, a test allows max(1, 2 x measured) ulp, and
nothing may exceed CAP = 16 ulp whatever was measured.  Texts with several operations: expr_reference.evaluate_with_bound
propagates these allowances through the text.  The scalar interpreter must give the per-DOF interpreter's BITS (same device
functions, no contraction across words in either).

`gaussian` is sqrt(-2 log u1) cos(tau u2) with tau the double nearest 2 pi.  Its error is counted in ulps of the RADIUS sqrt(-2 log u1),
not of the value: the product tau u2 is rounded to 2^-51 absolute, which near a zero of the cosine is any number of ulps of the value,
whatever the library does.

Every test prints what it measured (run with -s)."""
import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import expr_reference as R  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from oracle import expr_oracle as XO  # noqa: E402  (checker only)

CAP = 16.0
# largest ulp error against mpmath on an MI355X, inputs of expr_reference.TABLE; 'gaussian': see above
MEASURED_ULP = dict(sqrt=0.500, exp=0.655, log=0.565, sin=0.537, cos=0.483, tan=0.521, asin=0.565, acos=0.535, atan=0.970, sinh=0.506,
                    cosh=0.525, tanh=0.498, erf=0.601, erfc=1.294, POW=0.891, atan2=1.332, gaussian=3.626)
SHAPES = (1, 21, 22, 86)
SENTINEL = 12345.678
OPC = X.OPCODES
TAU = 6.283185307179586476925


def allowed(fn):
    return max(1.0, 2.0 * MEASURED_ULP[fn])


DEVICE = R.Budget(None, {fn: allowed(fn) for fn in R.MEASURED})


def word(op, arg=0):
    return OPC[op] | (int(arg) << 8)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


class Rig:
    """A context of n atoms with eight per-DOF operand buffers bound to slots 0..7."""

    def __init__(self, n):
        self.n, self.n3 = n, 3 * n
        self.ctx = B.HipContext(n, np.array([3.0, 3.0, 3.0]))
        new = lambda: torch.zeros((n, 3), dtype=torch.float64, device='cuda')        # noqa: E731
        self.x, self.v, self.mass = new(), new(), torch.ones(n, dtype=torch.float64, device='cuda')
        self.ctx.bind_state(self.x, self.v, self.mass)
        self.bufs = [new() for _ in range(8)]
        for k, buf in enumerate(self.bufs):
            self.ctx.bind_buffer(k, buf)
        self.out, self.total = new(), torch.zeros(1, dtype=torch.float64, device='cuda')

    def load(self, slot, values):
        """values cycled to fill the buffer"""
        self.bufs[slot].copy_(torch.as_tensor(np.resize(np.asarray(values, dtype=np.float64), self.n3).reshape(self.n, 3)))

    def launch(self, code, consts, gvals=(), seed=0, counter=0, total=False):
        self.out.fill_(SENTINEL)
        self.ctx.expr_eval(code, consts, list(gvals), seed, counter, dst=self.out, total=self.total if total else None)
        self.ctx.check()
        return self.out.cpu().numpy().reshape(-1).copy()

    def text(self, text, values, **kw):
        """Compile `text` (symbols p q r x y a b w u: buffers; anything else in values: a global) and run it."""
        names = [s for s in 'pqrxyabwu' if s in values]
        slot = {}

        def resolve(name):
            if name in names:
                return ('buf', slot.setdefault(name, len(slot)))
            return ('global',) if name in values else None
        prog = X.compile_per_dof(text, resolve)
        for name, k in slot.items():
            self.load(k, values[name])
        return self.launch(prog.code, prog.consts, [float(np.asarray(values[g]).reshape(-1)[0]) for g in prog.globals_], **kw)


_RIGS = {}


def rig(n):
    if n not in _RIGS:
        _RIGS[n] = Rig(n)
    return _RIGS[n]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for r in _RIGS.values():
        r.ctx.close()
    _RIGS.clear()
    _TABLE_RESULTS.clear()


# ------------------------------------------------------------------------------------------------ (a) every opcode of k_expr
_TABLE_RESULTS = {}


def table_result(name):
    """Device values of TABLE[name] by the per-DOF interpreter, one per input row (the rows cycled over 258 DOFs must all agree)."""
    if name not in _TABLE_RESULTS:
        rows = len(R.TABLE[name][1])
        assert rows <= 258
        got = rig(86).text(R.TABLE[name][0], R.table_values(name))
        assert all(same_bits(got[k], got[k % rows]) for k in range(len(got))), name
        _TABLE_RESULTS[name] = got[:rows]
    return _TABLE_RESULTS[name]


def check_table(name, got, label):
    """got (one value per row of TABLE[name]) against mpmath under the bound of the opcode; prints and returns the largest ulp error."""
    text, rows = R.TABLE[name]
    values = R.table_values(name)
    exact = R.evaluate(text, values)
    errors = [R.ulp_error(g, e) for g, e in zip(got, exact)]
    worst = max(errors)
    print('%s %-8s %-16s max ulp error %.3f at %r' % (label, name, text, worst, rows[int(np.argmax(errors))]))
    if name in R.MEASURED:
        assert worst <= allowed(name) and worst <= CAP, (name, worst, rows[int(np.argmax(errors))])
    else:
        bad = R.mismatches(got, R.evaluate_with_bound(text, values, DEVICE))
        assert bad == [], (name, [(rows[k], got[k], R.to_double(exact[k])) for k in bad])
    return worst


@pytest.mark.parametrize('name', sorted(R.TABLE))
def test_every_opcode_of_the_per_dof_interpreter(name):
    check_table(name, table_result(name), 'k_expr')


def test_edges_named_one_by_one():
    """The semantics the table must not lose silently if its rows are edited."""
    value = lambda name, row: float(table_result(name)[R.TABLE[name][1].index(row)])      # noqa: E731
    assert value('step', -0.0) == 1.0 and value('delta', -0.0) == 1.0 and value('step', -R.TINY) == 0.0 and value('delta', R.TINY) == 0.0
    assert value('select', (-0.0, 2.0, 3.0)) == 3.0 and value('select', (1.0, 2.0, 3.0)) == 2.0
    assert value('min', (3.0, 3.0)) == 3.0 and value('max', (3.0, 3.0)) == 3.0 and value('min', (2.0, 1.0)) == 1.0 and value('max', (1.0, 2.0)) == 2.0
    assert value('POW', (0.0, 0.0)) == 1.0 and value('POW', (-2.0, 2.0)) == 4.0 and value('POW', (-2.0, 3.0)) == -8.0
    assert math.isnan(value('POW', (-2.0, 0.5))) and math.isnan(value('sqrt', -1.0)) and math.isnan(value('asin', 2.0))
    assert math.copysign(1.0, R.TABLE['atan2'][1][6][0]) < 0                                  # (row 6 is (-0.0, -1): list.index cannot tell it from row 5)
    assert value('atan2', (0.0, -1.0)) == math.pi and float(table_result('atan2')[6]) == -math.pi and value('atan2', (-1.0, -2.0)) < -math.pi / 2
    assert value('floor', -0.5) == -1.0 and value('ceil', -0.5) == 0.0 and value('floor', 2.0 ** 52 + 1) == 2.0 ** 52 + 1
    assert value('POWI0', 0.0) == 1.0 and value('POWI-1', -2.0) == -0.5 and value('POWI-2', -2.0) == 0.25 and value('POWI3', -2.0) == -8.0
    assert value('SUB', (3.5, 1.25)) == 2.25 and value('DIV', (7.0, 2.0)) == 3.5


ARITHMETIC, TRANSCENDENTAL = 'p/q - r*p', 'exp(-p)*sin(q) + r'


@pytest.mark.parametrize('n', SHAPES)
@pytest.mark.parametrize('text', [ARITHMETIC, TRANSCENDENTAL])
def test_every_shape(n, text):
    """Distinct operands at every DOF: a wrong index shows as another DOF's value."""
    n3 = 3 * n
    values = dict(p=0.25 + 0.01 * np.arange(n3), q=1.5 + 0.003 * np.arange(n3)[::-1], r=np.cos(np.arange(n3)))
    got = rig(n).text(text, values)
    assert len(got) == n3 and R.mismatches(got, R.evaluate_with_bound(text, values, DEVICE)) == []


def test_scalar_only_words_are_refused_by_the_per_dof_entry():
    r = rig(1)
    for code in ([word('CONST'), word('OUT', 0)], [word('DEVG', 0)], [word('CONST'), word('HORNER', 0)]):
        r.out.fill_(SENTINEL)
        with pytest.raises(B.HipError):
            r.ctx.expr_eval(code, [1.0], [], 0, 0, dst=r.out)
        assert bool((r.out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ (b) ComputeSum
@pytest.mark.parametrize('n', SHAPES)
@pytest.mark.parametrize('case', ['products', 'cancelling'])
def test_compute_sum(n, case):
    """total against math.fsum of the device's own per-DOF values: only the reduction is under test.  Any order of summing n3 numbers
    is within n3 2^-53 sum|values| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, to first order)."""
    n3 = 3 * n
    k = np.arange(n3)
    if case == 'products':
        values = dict(p=0.25 + 0.01 * k, q=1.5 - 0.003 * k)
    else:
        values = dict(p=np.where(k % 2 == 0, 1e15, -1e15) + 0.37 * k, q=np.ones(n3))         # (an odd n3 leaves one 1e15 standing)
    r = rig(n)
    got = r.text('p*q', values, total=True)
    total = float(r.total.item())
    exact = math.fsum(got)
    bound = n3 * 2.0 ** -53 * math.fsum(abs(v) for v in got)
    print('sum n3 = %d %s: |total - fsum| = %.3e, bound %.3e' % (n3, case, abs(total - exact), bound))
    assert abs(total - exact) <= bound


# ------------------------------------------------------------------------------------------------ (c) limits of amm_expr_eval
def _sum_of(op, count):
    code = [word(op, 0)]
    for k in range(1, count):
        code += [word(op, k), word('ADD')]
    return code


def test_per_dof_program_limits_accepted():
    r = rig(1)
    numbers = [float(3 * k + 1) for k in range(48)]
    # exactly 256 words: c0 + 127 x c1, negated
    code = [word('CONST', 0)] + [word('CONST', 1), word('ADD')] * 127 + [word('NEG')]
    assert len(code) == 256 and np.all(r.launch(code, [0.5, 0.25]) == -(0.5 + 127 * 0.25))
    assert np.all(r.launch(_sum_of('CONST', 48), numbers) == sum(numbers))                       # 48 constants, the last one read
    assert np.all(r.launch(_sum_of('GLOBAL', 48), [], gvals=numbers) == sum(numbers))            # 48 globals
    # stack depth 24: a0 - (a1 - (a2 - ...)), every slot distinct
    deep = [1.0 / (k + 1) for k in range(24)]
    expect = deep[-1]
    for v in reversed(deep[:-1]):
        expect = v - expect
    assert np.all(r.launch([word('CONST', k) for k in range(24)] + [word('SUB')] * 23, deep) == expect)
    # 16 locals, each read back on its own
    store = list(itertools.chain.from_iterable((word('CONST', k), word('STORE', k)) for k in range(16)))
    for k in (0, 1, 7, 15):
        assert np.all(r.launch(store + [word('LOAD', k)], numbers[:16]) == numbers[k])


@pytest.mark.parametrize('what', ['257 words', '49 constants', '49 globals', 'depth 25', 'local 16 stored', 'local 16 loaded'])
def test_per_dof_program_limits_refused(what):
    r = rig(1)
    code, consts, gvals = [word('CONST', 0)], [1.0, 2.0], []
    if what == '257 words':
        code = [word('CONST', 0)] + [word('CONST', 1), word('ADD')] * 128
    elif what == '49 constants':
        consts = [1.0] * 49
    elif what == '49 globals':
        gvals = [1.0] * 49
    elif what == 'depth 25':
        code = [word('CONST', 0)] * 25 + [word('ADD')] * 24
    elif what == 'local 16 stored':
        code = [word('CONST', 0), word('STORE', 16), word('CONST', 0)]
    else:
        code = [word('LOAD', 16)]
    r.out.fill_(SENTINEL)
    with pytest.raises(B.HipError):
        r.ctx.expr_eval(code, consts, gvals, 0, 0, dst=r.out)
    r.ctx.check()
    assert bool((r.out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ (d) every opcode of k_expr_scalar
N_SCALARS = 4096


def opword(name):
    return word('POWI', int(name[4:])) if name.startswith('POWI') else word(name)


def rows_of(name):
    return [t if isinstance(t, tuple) else (t,) for t in R.TABLE[name][1]]


class Scalars:
    """The scalar buffer with the inputs of every table row laid out once: row i of TABLE[name] at `where[name, i]`..., outputs from `free`."""

    def __init__(self):
        self.ctx = rig(1).ctx
        host, self.where = [], {}
        for name in sorted(R.TABLE):
            for i, row in enumerate(rows_of(name)):
                self.where[name, i] = len(host)
                host += list(row)
        self.inputs = np.array(host, dtype=np.float64)
        self.free = len(host)
        assert self.free + 1200 < N_SCALARS
        self.reset()

    def reset(self):
        host = np.full(N_SCALARS, SENTINEL)
        host[:self.free] = self.inputs
        self.dev = torch.as_tensor(host, device='cuda')

    def snippet(self, name, i):
        return [word('DEVG', self.where[name, i] + j) for j in range(len(rows_of(name)[i]))] + [opword(name)]

    def run(self, code, consts=()):
        self.ctx.expr_eval_scalar(code, list(consts), self.dev)
        self.ctx.check()

    def host(self):
        return self.dev.cpu().numpy().copy()


@pytest.fixture(scope='module')
def scalars():
    return Scalars()


@pytest.mark.parametrize('name', sorted(R.TABLE))
def test_every_opcode_of_the_scalar_interpreter_one_assignment_per_launch(name, scalars):
    scalars.reset()
    rows = rows_of(name)
    for i in range(len(rows)):
        scalars.run(scalars.snippet(name, i) + [word('OUT', scalars.free + i)])
    host = scalars.host()
    got = host[scalars.free:scalars.free + len(rows)]
    assert same_bits(got, table_result(name)), (name, [(rows[k], got[k], table_result(name)[k]) for k in range(len(rows))
                                                          if not same_bits(got[k], table_result(name)[k])])
    check_table(name, got, 'k_expr_scalar')
    assert same_bits(host[:scalars.free], scalars.inputs) and bool(np.all(host[scalars.free + len(rows):] == SENTINEL))


FAST_PATH = ('CONST', 'MUL', 'ADD', 'LOAD', 'DEVG', 'SUB', 'HORNER')


def long_program(s):
    """One program of 600..640 words with every opcode of the scalar interpreter: assignments of table rows (operands by DEVG), and at
    each multiple of 64 an assignment laid so that a CONST is the last word of a chunk and a chosen opcode -- the seven of the fast path
    in front of the switch, then DIV and select from the switch -- the first word of the next.  Returns code, constants and
    [(destination, expected value or None, (table, row) or None)]."""
    code, consts, expect = [], [], []
    out = itertools.count(s.free)

    def const(v):
        consts.append(float(v))
        return word('CONST', len(consts) - 1)

    def close(value, source=None):
        dst = next(out)
        code.append(word('OUT', dst))
        expect.append((dst, value, source))

    order = sorted(s.where, key=lambda key: (key[1], key[0]))           # row 0 of every table first: every opcode early
    ordinary = itertools.cycle(order)
    a_in, b_in, c_in = s.where['SUB', 0], s.where['select', 2], s.where['DIV', 0]
    sv = lambda k: float(s.inputs[k])                # noqa: E731
    u, t, c = 0.7, 1.0 + 2.0 ** -30, -1.0

    def boundary(kind):
        """(words up to and including the CONST that ends the chunk, words after it, expected value)"""
        if kind == 'CONST':
            return [const(0.3)], [const(0.7), word('SUB')], 0.3 - 0.7
        if kind in ('MUL', 'ADD', 'SUB', 'DIV'):
            value = {'MUL': sv(a_in) * 0.3, 'ADD': sv(a_in) + 0.3, 'SUB': sv(a_in) - 0.3, 'DIV': sv(a_in) / 0.3}[kind]
            return [word('DEVG', a_in), const(0.3)], [word(kind)], value
        if kind == 'LOAD':
            return [const(0.9), word('STORE', 3), const(0.2)], [word('LOAD', 3), word('SUB')], 0.2 - 0.9
        if kind == 'DEVG':
            return [const(0.6)], [word('DEVG', c_in + 1), word('SUB')], 0.6 - sv(c_in + 1)
        if kind == 'HORNER':
            pre = [const(u), word('STORE', 0), const(t)]
            consts.append(c)
            return pre, [word('HORNER', len(consts) - 1)], R.fma(t, u, c)
        assert kind == 'select'                     # condition -0.0: the third operand
        return [word('DEVG', b_in), word('DEVG', b_in + 1), const(0.8)], [word('select')], 0.8

    for k, kind in enumerate(FAST_PATH + ('DIV', 'select'), start=1):
        pre, post, value = boundary(kind)
        target = 64 * k - len(pre)
        while True:
            name, i = key = next(ordinary)
            gap = target - (len(code) + len(s.snippet(name, i)) + 1)
            if gap < 0 or gap == 1:
                break
            code.extend(s.snippet(name, i))
            close(None, key)
        gap = target - len(code)
        assert gap == 0 or gap >= 2
        if gap:                                      # padding: an assignment of exactly `gap` words (x^1 is x)
            code.extend([const(0.125)] + [word('POWI', 1)] * (gap - 2))
            close(0.125)
        code.extend(pre)
        assert len(code) % 64 == 0 and (code[-1] & 0xff) == OPC['CONST'] and (post[0] & 0xff) == OPC[kind]
        code.extend(post)
        close(value)
    while True:
        name, i = key = next(ordinary)
        if len(code) + len(s.snippet(name, i)) + 1 > 640:
            break
        code.extend(s.snippet(name, i))
        close(None, key)
    return code, consts, expect


def test_long_scalar_program_with_words_on_both_sides_of_every_chunk_boundary(scalars):
    scalars.reset()
    code, consts, expect = long_program(scalars)
    assert 600 <= len(code) <= 640 and len(consts) <= 96
    used = {w & 0xff for w in code}
    per_dof_only = {OPC[k] for k in ('GLOBAL', 'BUF', 'MASS', 'GAUSS', 'UNIFORM')}
    assert used == set(OPC.values()) - per_dof_only, sorted(set(OPC.values()) - per_dof_only - used)
    for k in range(1, 10):
        assert (code[64 * k - 1] & 0xff) == OPC['CONST']
    assert [code[64 * k] & 0xff for k in range(1, 10)] == [OPC[k] for k in FAST_PATH + ('DIV', 'select')]
    scalars.run(code, consts)
    host = scalars.host()
    for dst, value, source in expect:
        want = table_result(source[0])[source[1]] if source else value
        assert same_bits(host[dst], want), (dst, source, host[dst], want)
    assert bool(np.all(host[expect[-1][0] + 1:] == SENTINEL)) and same_bits(host[:scalars.free], scalars.inputs)


def test_scalar_constants_stack_and_locals_by_lane(scalars):
    scalars.reset()
    f = scalars.free
    # every constant index, 0..63 in one register and 64..95 in the other
    consts = [k + 0.5 for k in range(96)]
    scalars.run(list(itertools.chain.from_iterable((word('CONST', k), word('OUT', f + k)) for k in range(96))), consts)
    assert same_bits(scalars.host()[f:f + 96], consts)
    # HORNER's constant from both registers: 2 * 3 + c
    scalars.run([word('CONST', 3), word('STORE', 0), word('CONST', 2), word('HORNER', 63), word('OUT', f + 100),
                 word('CONST', 2), word('HORNER', 64), word('OUT', f + 101), word('CONST', 2), word('HORNER', 95), word('OUT', f + 102)], consts)
    assert same_bits(scalars.host()[f + 100:f + 103], [3.5 * 2.5 + 63.5, 3.5 * 2.5 + 64.5, 3.5 * 2.5 + 95.5])
    # stack depth 24, right-nested: a0 - (a1 - (a2 - ...))
    deep = [1.0 / (k + 1) for k in range(24)]
    expect = deep[-1]
    for v in reversed(deep[:-1]):
        expect = v - expect
    scalars.run([word('CONST', k) for k in range(24)] + [word('SUB')] * 23 + [word('OUT', f + 110)], deep)
    assert same_bits(scalars.host()[f + 110], expect)
    # ... and through the switch (DIV), so that both pop orders are seen
    expect = deep[-1]
    for v in reversed(deep[:-1]):
        expect = v / expect
    scalars.run([word('CONST', k) for k in range(24)] + [word('DIV')] * 23 + [word('OUT', f + 111)], deep)
    assert same_bits(scalars.host()[f + 111], expect)
    # all 16 locals
    code = list(itertools.chain.from_iterable((word('CONST', k), word('STORE', k)) for k in range(16)))
    code += list(itertools.chain.from_iterable((word('LOAD', k), word('OUT', f + 120 + k)) for k in range(16)))
    scalars.run(code, consts)
    assert same_bits(scalars.host()[f + 120:f + 136], consts[:16])
    scalars.run([word('CONST', 5), word('STORE', 0), word('CONST', 9), word('STORE', 15), word('LOAD', 15), word('LOAD', 0), word('SUB'),
                 word('OUT', f + 140)], consts)
    assert scalars.host()[f + 140] == 9.5 - 5.5


def test_scalar_assignments_read_earlier_ones(scalars):
    scalars.reset()
    f = scalars.free
    scalars.dev[f] = 0.3
    step = lambda k: [word('DEVG', f + k), word('CONST', 0), word('MUL'), word('CONST', 1), word('ADD'), word('OUT', f + k + 1)]      # noqa: E731
    scalars.run(list(itertools.chain.from_iterable(step(k) for k in range(10))), [1.5, 0.1])        # ten in one launch
    expect = [0.3]
    for _ in range(20):
        expect.append(expect[-1] * 1.5 + 0.1)
    assert same_bits(scalars.host()[f:f + 11], expect[:11])
    scalars.run(list(itertools.chain.from_iterable(step(k) for k in range(10, 20))), [1.5, 0.1])    # a second launch reads the first's
    assert same_bits(scalars.host()[f:f + 21], expect)


def test_scalar_polynomial_and_predicated_assignment(scalars):
    scalars.reset()
    f = scalars.free
    scalars.dev[f:f + 4] = torch.as_tensor([0.25, -12.5, 4.0, 1.0], device='cuda')
    coef = [float(v) for v in np.random.default_rng(1).normal(size=9)]
    prog = X.compile_polynomial(coef, 2.0, -1.0, X.Deferred(0.6, {f: 0.5}))
    scalars.run(prog.code + [word('OUT', f + 10)], prog.consts)
    u = (0.6 + 0.25 * 0.5) * 2.0 + -1.0
    acc = coef[-1]
    for c in reversed(coef[:-1]):
        acc = R.fma(acc, u, c)
    assert sum((w & 0xff) == OPC['HORNER'] for w in prog.code) == 8
    assert same_bits(scalars.host()[f + 10], acc)
    # target <- select(condition, expression, target), the condition on the device: both directions
    v = X.Deferred(0.05, {f + 1: -1e-5, f + 2: 2e-5})
    number = (0.05 + -12.5 * -1e-5) + 4.0 * 2e-5
    for cond_at, want in ((f + 3, -number), (f + 4, number)):
        scalars.dev[f + 4] = 0.0
        prog = X.compile_scalar('-_v', {'_v': v}, None, X.Deferred(0.0, {cond_at: 1.0}), v)
        scalars.run(prog.code + [word('OUT', f + 11)], prog.consts)
        assert same_bits(scalars.host()[f + 11], want)


def test_scalar_program_limits(scalars):
    scalars.reset()
    f = scalars.free
    scalars.run([word('CONST', 95)] + [word('POWI', 1)] * 638 + [word('OUT', f)], [float(k) for k in range(96)])     # 640 words, 96 constants
    assert scalars.host()[f] == 95.0
    before = scalars.host()
    refused = {
        '641 words': ([word('CONST', 0)] + [word('POWI', 1)] * 639 + [word('OUT', f)], [1.0]),
        '97 constants': ([word('CONST', 0), word('OUT', f)], [1.0] * 97),
        'OUT at depth 2': ([word('CONST', 0), word('CONST', 0), word('OUT', f), word('OUT', f)], [1.0]),
        'OUT at depth 0': ([word('CONST', 0), word('OUT', f), word('OUT', f)], [1.0]),
        'depth 25': ([word('CONST', 0)] * 25 + [word('ADD')] * 24 + [word('OUT', f)], [1.0]),
        'no assignment': ([word('CONST', 0), word('STORE', 0)], [1.0]),
        'value left over': ([word('CONST', 0), word('OUT', f), word('CONST', 0)], [1.0]),
        'destination out of range': ([word('CONST', 0), word('OUT', N_SCALARS)], [1.0]),
        'operand out of range': ([word('DEVG', N_SCALARS), word('OUT', f)], [1.0]),
    }
    for op in ('BUF', 'MASS', 'GLOBAL', 'GAUSS', 'UNIFORM'):
        refused['per-DOF operand ' + op] = ([word(op, 0), word('OUT', f)], [1.0])
    for what, (code, consts) in refused.items():
        with pytest.raises(B.HipError, match='amm_expr_eval_scalar'):              # (pytest names `what` through the loop variable on failure)
            scalars.ctx.expr_eval_scalar(code, consts, scalars.dev)
    scalars.ctx.check()
    assert same_bits(scalars.host(), before)


# ------------------------------------------------------------------------------------------------ (e) text to device
CORPUS_SEED, CORPUS_COUNTER = 2 ** 40 + 11, 2 ** 63 + 5


@pytest.fixture(scope='module')
def corpus_inputs():
    """The corpus inputs at 22 atoms; `c` and `lambda` travel as globals (one number for every DOF); gaussian and uniform are the
    device's own draws of the launch (section (f) checks the stream itself)."""
    values = R.corpus_values(66)
    values['c'] = np.full(66, values['c'][0])
    values['lambda'] = np.full(66, values['lambda'][0])
    values['gaussian'] = rig(22).text('gaussian', {}, seed=CORPUS_SEED, counter=CORPUS_COUNTER)
    values['uniform'] = rig(22).text('uniform', {}, seed=CORPUS_SEED, counter=CORPUS_COUNTER)
    return values


@pytest.mark.parametrize('text', R.CORPUS)
def test_corpus_text_to_device(text, corpus_inputs):
    got = rig(22).text(text, corpus_inputs, seed=CORPUS_SEED, counter=CORPUS_COUNTER)
    reference = R.evaluate_with_bound(text, corpus_inputs, DEVICE)
    bad = R.mismatches(got, reference)
    assert bad == [], (text, [(k, got[k], R.ulp_error(got[k], reference[k][0])) for k in bad[:5]])


# ------------------------------------------------------------------------------------------------ (f) random stream
SEEDS = (3, 2 ** 32 + 5, 2 ** 64 - 1)
COUNTERS = (7, 2 ** 32 + 7, 2 ** 63 + 9)


def philox_words(n3, occurrence, seed, counter):
    """The two 53-bit integers of every DOF, from the oracle's round function alone."""
    full = lambda v: np.full(n3, v, dtype=np.uint64)      # noqa: E731
    r = XO.philox4x32_10(np.arange(n3, dtype=np.uint64), full(occurrence), full(counter & 0xFFFFFFFF), full(counter >> 32),
                         seed & 0xFFFFFFFF, seed >> 32)
    mask = np.uint64((1 << 53) - 1)
    return ((r[0] << np.uint64(21)) ^ (r[1] >> np.uint64(11))) & mask, ((r[2] << np.uint64(21)) ^ (r[3] >> np.uint64(11))) & mask


def check_uniform(u, n3, seed, counter):
    """u = (word + 1/2) 2^-53 for the oracle's 53-bit word.  Below 2^52 the sum is a double and u * 2^53 - 1/2 gives the word back,
    exactly.  From 2^52 on word + 1/2 has 54 bits and no double holds it (so no implementation can return the word there): the device
    must then give the nearest double, ties to even -- the word if it is even, the word + 1 if it is odd."""
    words = philox_words(n3, 1, seed, counter)[0]
    small = words < np.uint64(1 << 52)
    assert small.any() and (~small).any()
    a = u * 2.0 ** 53 - 0.5
    assert np.all(a[small] == np.floor(a[small])) and np.array_equal(a[small].astype(np.uint64), words[small])
    scaled = u * 2.0 ** 53                            # (a power of two: exact)
    assert np.array_equal(scaled[~small].astype(np.uint64), words[~small] + (words[~small] & np.uint64(1)))
    assert np.all(u > 0.0) and np.all(u <= 1.0)


def gaussian_errors(g, dofs, n3, seed, counter):
    """|g - sqrt(-2 log u1) cos(TAU u2)| in ulps of the radius, for the DOFs listed; u1, u2: the oracle's two uniforms (doubles)."""
    u1, u2 = XO.uniforms(n3, 0, seed, counter)
    a, b = philox_words(n3, 0, seed, counter)
    assert np.array_equal(u1, (a.astype(np.float64) + 0.5) * 2.0 ** -53) and np.array_equal(u2, (b.astype(np.float64) + 0.5) * 2.0 ** -53)
    errors = []
    with R.mpmath.workdps(R.DIGITS):
        for k in dofs:
            radius = R.mpmath.sqrt(-2 * R.mpmath.log(R.mpf(float(u1[k]))))
            errors.append(float(abs(R.mpf(float(g[k])) - radius * R.mpmath.cos(R.mpf(TAU) * R.mpf(float(u2[k])))) / R.ulp(radius)))
    return errors


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('counter', COUNTERS)
def test_random_stream(seed, counter):
    r = rig(22)
    u = r.text('uniform', {}, seed=seed, counter=counter)
    check_uniform(u, 66, seed, counter)
    g = r.text('gaussian', {}, seed=seed, counter=counter)
    worst = max(gaussian_errors(g, range(66), 66, seed, counter))
    print('gaussian seed %#x counter %#x: max error %.3f ulp of the radius' % (seed, counter, worst))
    assert worst <= allowed('gaussian') and worst <= CAP
    assert np.all(r.text('gaussian - gaussian', {}, seed=seed, counter=counter) == 0.0)
    assert np.all(r.text('g1 - g2; g1 = gaussian; g2 = gaussian', {}, seed=seed, counter=counter) == 0.0)
    assert same_bits(r.text('gaussian*4 + uniform', {}, seed=seed, counter=counter), g * 4 + u)
    assert not np.array_equal(g, r.text('gaussian', {}, seed=seed, counter=counter + 1))


def test_random_stream_beyond_65536_degrees_of_freedom():
    n = 21846
    big = Rig(n)
    try:
        seed, counter = SEEDS[1], COUNTERS[2]
        u = big.text('uniform', {}, seed=seed, counter=counter)
        check_uniform(u, 3 * n, seed, counter)
        g = big.text('gaussian', {}, seed=seed, counter=counter)
        dofs = list(range(16)) + list(range(65528, 3 * n))
        worst = max(gaussian_errors(g, dofs, 3 * n, seed, counter))
        print('gaussian at DOFs up to %d: max error %.3f ulp of the radius' % (3 * n - 1, worst))
        assert worst <= allowed('gaussian') and worst <= CAP
        # ... and every DOF against the oracle's numpy Box-Muller: each side is within CAP ulps of the radius of the exact value
        u1, u2 = XO.uniforms(3 * n, 0, seed, counter)
        ref = np.sqrt(-2.0 * np.log(u1)) * np.cos(TAU * u2)
        assert np.all(np.abs(g - ref) <= 32 * np.spacing(np.sqrt(-2.0 * np.log(u1))))
    finally:
        big.ctx.close()
