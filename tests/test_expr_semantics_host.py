"""What an expression TEXT means, on every host path, against the independent mpmath evaluator of tests/expr_reference.py: the
compiler of atomsmm_amd/expr.py followed by the numpy restatement of the per-DOF interpreter (oracle/expr_oracle.py), the host's
own evaluator (eval_global), and compile_scalar followed by the word-by-word runner of the scalar interpreter (tests/scalar_runner.py).
The Philox round function of the oracle -- and through tests/test_gpu_expr_opcodes.py that of the device -- is anchored to the
published known-answer vectors of Philox-4x32-10 (Random123, kat_vectors).

Bounds: the correctly rounded operations 0.5 ulp, every library function 4 ulp (numpy, scipy.special, math), propagated through the
text by expr_reference.evaluate_with_bound.  test_numpy_meets_the_host_bound_on_every_table_input checks the 4 ulp on the opcode
tables the device tests use; HOST_REMOVED lists the inputs at which numpy / scipy miss it (none may exceed 5 % of a function's list)."""
import math

import numpy as np
import pytest

import expr_reference as R
import scalar_runner as SR
from atomsmm_amd import expr as X
from oracle import expr_oracle as XO

HOST = R.Budget(4, powi_counts=False)
# inputs of expr_reference.TABLE at which numpy / scipy are more than 4 ulp from the exact value: scipy.special.erfc is 4.1 ulp off at
# 26.6 (a subnormal result) and 6.4 ulp at 2.857 (math.erfc: 0.1 and 0.4); 2 of erfc's 40 inputs.  The device tests keep both.
HOST_REMOVED = {'erfc': [(26.6,), (2.857,)]}


def _hex(words):
    return ' '.join('%08x' % int(w) for w in words)


@pytest.mark.parametrize('counter,key,expected', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, expected):
    assert _hex(XO.philox4x32_10(*counter, *key)) == expected
    # ... and element-wise on arrays, as uniforms() calls it
    out = XO.philox4x32_10(*[np.array([c, 0], dtype=np.uint64) for c in counter], *key)
    assert _hex(w[0] for w in out) == expected


VALUES = R.corpus_values(51)              # 17 atoms x 3


class _Draws:
    """Stands in for the numpy Generator of eval_global / compile_scalar: hands out the corpus' own draws."""

    def __init__(self, k):
        self.k = k

    def standard_normal(self):
        return VALUES['gaussian'][self.k]

    def random(self):
        return VALUES['uniform'][self.k]


def _row(k):
    return {name: float(v[k]) for name, v in VALUES.items() if name not in ('gaussian', 'uniform')}


@pytest.fixture(scope='module')
def corpus_reference():
    return {text: R.evaluate_with_bound(text, VALUES, HOST) for text in R.CORPUS}


def test_the_corpus_covers_what_it_should():
    text = ' ; '.join(R.CORPUS)
    for fn in X.OPCODES:
        if not fn.isupper():
            assert fn + '(' in text, fn
    for piece in ('-x^2', '2^-x', 'x^-2^2', 'x^y^2', 'a-b-c', 'a/b/c', 'a/b*c', '-a*b', 'a--b', 'x^2.0', 'x^-2', 'x^(-2)', 'x^0', 'x^1', 'x^0.5',
                  '^1048576', '1E-3*x', '.5*x', 'lambda', 'gaussian - gaussian'):
        assert any(piece in t for t in R.CORPUS), piece
    assert len(VALUES['x']) >= 50


def test_reference_reads_the_grammar_as_stated():
    one = lambda text, **kw: R.evaluate(text, kw)[0]       # noqa: E731
    assert one('-x^2', x=3.0) == -9 and one('2^-x', x=2.0) == 0.25 and one('x^-2^2', x=2.0) == 0.0625 and one('x^y^2', x=2.0, y=3.0) == 512
    assert one('a-b-c', a=1.0, b=2.0, c=4.0) == -5 and one('a/b/c', a=8.0, b=2.0, c=4.0) == 1 and one('a/b*c', a=8.0, b=2.0, c=4.0) == 16
    assert one('-a*b', a=2.0, b=3.0) == -6 and one('a--b', a=2.0, b=3.0) == 5 and one('2*-x', x=3.0) == -6
    assert one('1.', x=0.0) == 1 and one('.5', x=0.0) == 0.5 and one('1E8', x=0.0) == 10 ** 8 and R.to_double(one('1e-3', x=0.0)) == 1e-3
    assert one('select(c, a, b)', c=0.0, a=1.0, b=2.0) == 2 and one('atan2(a, b)', a=1.0, b=0.0) > 1.5
    assert one('r + s; s = r*2; r = x', x=1.5) == 4.5
    assert math.isnan(R.to_double(one('(0-2)^0.5', x=0.0))) and math.isnan(R.to_double(one('sqrt(x)', x=-1.0)))
    assert R.to_double(one('exp(x)', x=1000.0)) == math.inf and R.to_double(one('-exp(x)', x=1000.0)) == -math.inf
    assert R.to_double(R.mpf(2) ** -1074 * 0.75) == 5e-324 and R.ulp_error(1.0 + 2.0 ** -52, 1) == 1.0
    assert R.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60            # (the two-step result is 0)
    for bad in ('foo(x)', 'min(x)', 'a +', 'a; a = b; b = a', '(x'):
        with pytest.raises(R.ParseError):
            R.evaluate(bad, dict(x=1.0))


@pytest.mark.parametrize('text', R.CORPUS)
def test_corpus_compiled_per_dof_and_run_by_the_oracle(text, corpus_reference):
    n = len(VALUES['x']) // 3
    names = [k for k in VALUES if k not in ('gaussian', 'uniform', 'lambda', 'c')]
    slots = {name: k for k, name in enumerate(names)}
    seed, counter = 2 ** 40 + 11, 2 ** 63 + 5

    def resolve(name):
        if name in slots:
            return ('buf', slots[name])
        return ('global',) if name in ('lambda', 'c') else None
    prog = X.compile_per_dof(text, resolve)
    # `lambda` and `c` travel as per-launch globals, which are one number for all DOFs: run DOF by DOF groups of equal globals
    u1, u2 = XO.uniforms(3 * n, 0, seed, counter)
    values = dict(VALUES)
    values['gaussian'] = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)
    values['uniform'] = XO.uniforms(3 * n, 1, seed, counter)[0]
    uses_globals = bool(prog.globals_)
    reference = R.evaluate_with_bound(text, values, HOST) if ('gaussian' in text or 'uniform' in text) else corpus_reference[text]
    bufs = {slots[name]: np.asarray(VALUES[name]).reshape(n, 3) for name in names}
    with np.errstate(all='ignore'):
        if not uses_globals:
            got = XO.run(prog.code, prog.consts, [], bufs, np.ones(n), seed, counter).reshape(-1)
        else:
            got = np.array([XO.run(prog.code, prog.consts, [VALUES[g][k] for g in prog.globals_], bufs, np.ones(n), seed, counter).reshape(-1)[k]
                            for k in range(3 * n)])
    assert R.mismatches(got, reference) == []


@pytest.mark.parametrize('text', R.CORPUS)
def test_corpus_evaluated_by_eval_global(text, corpus_reference):
    got = [X.eval_global(text, _row(k), _Draws(k)) for k in range(len(VALUES['x']))]
    assert R.mismatches(got, corpus_reference[text]) == []


@pytest.mark.parametrize('text', R.CORPUS)
def test_corpus_compiled_to_a_scalar_program(text, corpus_reference):
    """Every symbol as a Deferred, so that its value reaches the program through DEVG words."""
    names = [k for k in VALUES if k not in ('gaussian', 'uniform')]
    env = {name: X.Deferred(0.0, {k: 1.0}) for k, name in enumerate(names)}
    got = []
    for k in range(len(VALUES['x'])):
        prog = X.compile_scalar(text, env, _Draws(k))
        got.append(SR.evaluate(prog, {j: float(VALUES[name][k]) for j, name in enumerate(names)}))
    assert R.mismatches(got, corpus_reference[text]) == []


@pytest.mark.parametrize('text', [
    'a; a = b + 1; b = a*2',                                                       # circular
    '+'.join('d%d' % k for k in range(17)) + ''.join('; d%d = x+%d' % (k, k) for k in range(17)),      # a 17th definition
    'foo(x)',                                                                      # unknown function
    'min(x)', 'sqrt(x, y)', 'select(x, y)', 'atan2(x)',                            # wrong arity
    'x + nosuch',                                                                  # unknown symbol
])
def test_errors(text):
    with pytest.raises(X.ExpressionError):
        X.compile_per_dof(text, lambda name: ('buf', 0) if name in ('x', 'y') else None)
    with pytest.raises(X.ExpressionError):
        X.compile_scalar(text, dict(x=1.0, y=2.0))
    if 'd16' not in text:                            # (the host evaluator keeps definitions in a dictionary: no limit to reach)
        with pytest.raises(X.ExpressionError):
            X.eval_global(text, dict(x=1.0, y=2.0))


def test_sixteen_definitions_are_accepted():
    text = '+'.join('d%d' % k for k in range(16)) + ''.join('; d%d = x+%d' % (k, k) for k in range(16))
    prog = X.compile_per_dof(text, lambda name: ('buf', 0))
    assert max(w >> 8 for w in prog.code if (w & 0xff) == X.OPCODES['STORE']) == 15
    got = XO.run(prog.code, prog.consts, [], {0: np.full((1, 3), 0.25)}, np.ones(1), 0, 0).reshape(-1)
    assert got[0] == 16 * 0.25 + sum(range(16))


def _table_run(name):
    text = R.TABLE[name][0]
    count = -(-len(R.TABLE[name][1]) // 3) * 3
    values = R.table_values(name, count)
    prog = X.compile_per_dof(text, lambda s: ('buf', 'pqr'.index(s)) if s in 'pqr' else None)
    bufs = {j: np.array(values[s]).reshape(-1, 3) for j, s in enumerate('pqr')}
    with np.errstate(all='ignore'):
        got = XO.run(prog.code, prog.consts, [], bufs, np.ones(count // 3), 0, 0).reshape(-1)
    return prog, values, got


@pytest.mark.parametrize('name', sorted(R.TABLE))
def test_numpy_meets_the_host_bound_on_every_table_input(name):
    prog, values, got = _table_run(name)
    reference = R.evaluate_with_bound(R.TABLE[name][0], values, HOST)
    removed = HOST_REMOVED.get(name, [])
    assert len(removed) <= 0.05 * len(R.TABLE[name][1])
    arity = len(removed[0]) if removed else 3
    bad = sorted({tuple(values[s][k] for s in 'pqr')[:arity] for k in R.mismatches(got, reference)} - set(removed))
    assert bad == []


# opcodes both interpreters' restatements support, with operands at which math.* does not raise
AGREE = dict(ADD=[(0.1, 0.2), (3.5, -1.25)], SUB=[(3.5, 1.25), (0.1, 0.3)], MUL=[(0.1, 0.3), (-3.0, 7.0)], DIV=[(1.0, 3.0), (2.0, -7.0)],
             NEG=[(0.3,), (-2.0,)], POW=[(2.0, 0.5), (10.0, 2.5), (-2.0, 3.0), (0.3, -0.7)], min=[(1.0, 2.0), (2.0, 1.0)], max=[(1.0, 2.0), (2.0, 1.0)],
             atan2=[(1.0, -2.0), (-1.0, 2.0)], select=[(1.0, 2.0, 3.0), (0.0, 2.0, 3.0), (-0.0, 2.0, 3.0)],
             **{fn: [(0.3,), (0.9,), (-0.45,)] for fn in SR.FUN if fn not in ('sqrt', 'log')}, sqrt=[(0.3,), (2.0,)], log=[(0.3,), (2.0,)])
EXACT_OPS = ('ADD', 'SUB', 'MUL', 'DIV', 'NEG', 'abs', 'floor', 'ceil', 'step', 'delta', 'min', 'max', 'select')


def _both(word, operands):
    consts = list(operands)
    code = [X.OPCODES['CONST'] | (k << 8) for k in range(len(consts))] + [word]
    with np.errstate(all='ignore'):
        per_dof = XO.run(code, consts, [], {}, np.ones(1), 0, 0).reshape(-1)[0]
    scalars = {}
    SR.run(code + [X.OPCODES['OUT'] | (5 << 8)], consts, scalars)
    return float(per_dof), float(scalars[5])


@pytest.mark.parametrize('op', sorted(AGREE))
def test_the_two_restatements_agree(op):
    """oracle.expr_oracle.run (k_expr) and scalar_runner.run (k_expr_scalar): equal bits for the correctly rounded operations, within
    twice the host bound of each other (each is within 4 ulp of the exact value) for library functions."""
    for operands in AGREE[op]:
        a, b = _both(X.OPCODES[op], operands)
        if op in EXACT_OPS:
            assert a == b, (op, operands, a, b)
        else:
            assert abs(a - b) <= 8 * float(R.ulp(a)), (op, operands, a, b)


@pytest.mark.parametrize('n', [0, 1, 2, 3, 7, 64, -1, -2, -7])
def test_the_two_restatements_agree_on_integer_powers(n):
    for base in (1.5, -1.5, 0.999, -0.7, 3.0):
        a, b = _both(X.OPCODES['POWI'] | (n << 8), (base,))
        exact = R.mpf(base) ** n
        assert R.ulp_error(a, exact) <= 4 and R.ulp_error(b, exact) <= 4, (n, base, a, b)
        assert (a < 0) == (b < 0) == (exact < 0)
