"""TEST INFRASTRUCTURE (checker only): an evaluator of OpenMM expression TEXT that shares nothing with atomsmm_amd/expr.py -- its
own tokenizer, its own recursive-descent parser, mpmath at 50 digits -- so that a mistake of the compiler (operand order, precedence,
a definition bound to the wrong local) shows as a different number, which the postfix restatements of the interpreters cannot see.

Grammar (lowest to highest precedence): `+ -`, `* /`, unary minus, `^` (right-associative, its exponent may itself begin with a
minus sign: `2^-x`, `x^-2^2` = x^(-(2^2))); functions with fixed arities; numbers `1`, `1.`, `.5`, `1e-3`, `1E8`; auxiliary
definitions `; name = expression` after the main expression, in any order.

Values: a real result that does not exist (sqrt(-1), (-2)^0.5, log(-1), asin(2)) is NaN, a pole is +inf, and to_double() turns what
exceeds the double range into +-inf.  mpmath has no signed zero, so neither has this evaluator (but for atan2(-0, negative) = -pi).

Error bounds: evaluate_with_bound() returns with every value a bound on the distance of a DOUBLE evaluation of the same text from
it, by first-order forward error analysis: every node adds `ulps(node) * ulp(value)` to what its operands' errors become through
the node's partial derivatives (taken at the operand and at both ends of the operand's error interval).  A node whose result could
jump inside that interval (floor, step, a select condition, a division by something that may be zero) raises Unstable: such an input
checks nothing and is to be replaced."""
import fractions
import math
import re

import mpmath
from mpmath import mpf

DIGITS = 50
FUNCTIONS = dict(sqrt=1, exp=1, log=1, sin=1, cos=1, tan=1, asin=1, acos=1, atan=1, sinh=1, cosh=1, tanh=1, erf=1, erfc=1, abs=1,
                 floor=1, ceil=1, step=1, delta=1, min=2, max=2, select=3, atan2=2)
EXACT = ('+', '-', '*', '/', 'neg', 'abs', 'floor', 'ceil', 'step', 'delta', 'min', 'max', 'select')      # correctly rounded on every path
POWI_LIMIT = 1 << 20        # |integer literal exponent| below this: repeated multiplication, relative error <= |e| 2^-52


class ParseError(ValueError):
    pass


class Unstable(ValueError):
    """The value of the text is discontinuous within the rounding error of its operands at this input."""


# ---------------------------------------------------------------------------------------------------------------- numbers
def to_double(x):
    """The double nearest to x (ties to even), +-inf beyond the double range, nan for nan."""
    x = mpf(x)
    if mpmath.isnan(x):
        return math.nan
    if mpmath.isinf(x):
        return math.inf if x > 0 else -math.inf
    sign, man, exp, _ = x._mpf_
    if man == 0:
        return 0.0
    try:
        value = float(man << exp) if exp >= 0 else man / (1 << -exp)     # int -> float and int / int round correctly, subnormals included
    except OverflowError:
        value = math.inf
    return -value if sign else value


def ulp(x):
    """Spacing of the doubles in the binade of |x| (that of the subnormals below the smallest normal)."""
    x = abs(mpf(x))
    if x == 0 or mpmath.isnan(x) or mpmath.isinf(x):
        return mpf(2) ** -1074
    e = max(int(mpmath.floor(mpmath.log(x, 2))), -1022)
    while mpf(2) ** e > x and e > -1022:          # (log2 of a number a hair below a power of two may round up)
        e -= 1
    while mpf(2) ** (e + 1) <= x:
        e += 1
    return mpf(2) ** (e - 52)


def ulp_error(got, exact):
    """|got - exact| in units of ulp(exact); 0 where both are nan or the same infinity, inf where only one is."""
    with mpmath.workdps(DIGITS):
        exact = mpf(exact)
        got = float(got)
        if mpmath.isnan(exact) or math.isnan(got):
            return 0.0 if mpmath.isnan(exact) and math.isnan(got) else math.inf
        rounded = to_double(exact)
        if math.isinf(rounded) or math.isinf(got):
            return 0.0 if rounded == got else math.inf
        return float(abs(mpf(got) - exact) / ulp(exact))


def fma(a, b, c):
    """a * b + c rounded once."""
    if any(math.isnan(v) or math.isinf(v) for v in (a, b, c)):
        return a * b + c
    exact = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    if exact == 0:
        return a * b + c                           # (the sign of an exact zero: as the plain operations give it)
    try:
        return exact.numerator / exact.denominator
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


# ---------------------------------------------------------------------------------------------------------------- parser
_TOKEN = re.compile(r'\s*(?:(?P<num>(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)|(?P<name>[A-Za-z_][A-Za-z_0-9]*)|(?P<op>[-+*/^(),]))')


def _tokens(text):
    out, pos = [], 0
    text = text.rstrip()
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            raise ParseError('cannot read %r at %r' % (text, text[pos:]))
        out.append((m.lastgroup, m.group(m.lastgroup)))
        pos = m.end()
    return out


class _Parser:
    def __init__(self, text):
        self.toks, self.k, self.text = _tokens(text), 0, text

    def peek(self):
        return self.toks[self.k] if self.k < len(self.toks) else (None, None)

    def take(self, value=None):
        kind, tok = self.peek()
        if kind is None or (value is not None and tok != value):
            raise ParseError('expected %r in %r' % (value or 'more', self.text))
        self.k += 1
        return kind, tok

    def parse(self):
        node = self.sum()
        if self.k != len(self.toks):
            raise ParseError('trailing %r in %r' % (self.peek()[1], self.text))
        return node

    def sum(self):
        node = self.product()
        while self.peek() in (('op', '+'), ('op', '-')):
            op = self.take()[1]
            node = ('bin', op, node, self.product())
        return node

    def product(self):
        node = self.unary()
        while self.peek() in (('op', '*'), ('op', '/')):
            op = self.take()[1]
            node = ('bin', op, node, self.unary())
        return node

    def unary(self):
        if self.peek() == ('op', '-'):
            self.take()
            return ('neg', self.unary())
        if self.peek() == ('op', '+'):
            self.take()
            return self.unary()
        return self.power()

    def power(self):
        base = self.atom()
        if self.peek() == ('op', '^'):
            self.take()
            return ('bin', '^', base, self.unary())           # right-associative; the exponent may carry its own sign
        return base

    def atom(self):
        kind, tok = self.take()
        if kind == 'num':
            return ('num', tok)
        if kind == 'name':
            if self.peek() == ('op', '('):
                self.take()
                args = [self.sum()]
                while self.peek() == ('op', ','):
                    self.take()
                    args.append(self.sum())
                self.take(')')
                if tok not in FUNCTIONS:
                    raise ParseError('unknown function %s in %r' % (tok, self.text))
                if len(args) != FUNCTIONS[tok]:
                    raise ParseError('%s takes %d arguments: %r' % (tok, FUNCTIONS[tok], self.text))
                return ('call', tok, args)
            return ('var', tok)
        if tok == '(':
            node = self.sum()
            self.take(')')
            return node
        raise ParseError('unexpected %r in %r' % (tok, self.text))


def parse(text):
    """(main tree, {name: tree}) of `main; name = expression; ...`."""
    parts = [p for p in text.split(';') if p.strip()]
    if not parts:
        raise ParseError('empty expression')
    defs = {}
    for p in parts[1:]:
        if '=' not in p:
            raise ParseError('definition without "=": ' + p)
        name, rhs = p.split('=', 1)
        defs[name.strip()] = _Parser(rhs).parse()
    return _Parser(parts[0]).parse(), defs


# ---------------------------------------------------------------------------------------------------------------- evaluation
def _real(f, *args):
    """f(*args) where it is real: nan where mpmath answers with a complex number or refuses, +inf at a pole."""
    try:
        v = f(*args)
    except ZeroDivisionError:
        return mpmath.inf
    except (ValueError, TypeError):
        return mpmath.nan
    if isinstance(v, mpmath.mpc):
        return v.real if v.imag == 0 else mpmath.nan
    return v


def _power(a, b):
    if a == 0 and b == 0:
        return mpf(1)
    if a == 0 and b < 0:
        return mpmath.inf
    if a < 0 and b != mpmath.floor(b):
        return mpmath.nan
    return _real(mpmath.power, a, b)


_UNARY = dict(
    sqrt=lambda x: mpmath.nan if x < 0 else mpmath.sqrt(x), exp=mpmath.exp, log=lambda x: mpmath.nan if x < 0 else (-mpmath.inf if x == 0 else mpmath.log(x)),
    sin=mpmath.sin, cos=mpmath.cos, tan=mpmath.tan, asin=lambda x: mpmath.nan if abs(x) > 1 else mpmath.asin(x),
    acos=lambda x: mpmath.nan if abs(x) > 1 else mpmath.acos(x), atan=mpmath.atan, sinh=mpmath.sinh, cosh=mpmath.cosh, tanh=mpmath.tanh,
    erf=mpmath.erf, erfc=mpmath.erfc, abs=abs, floor=mpmath.floor, ceil=mpmath.ceil, step=lambda x: mpf(1 if x >= 0 else 0),
    delta=lambda x: mpf(1 if x == 0 else 0))
# |d f / d x|, for the propagation of an operand's error
_SLOPE = dict(
    sqrt=lambda x: 1 / (2 * mpmath.sqrt(x)), exp=mpmath.exp, log=lambda x: 1 / abs(x), sin=lambda x: abs(mpmath.cos(x)),
    cos=lambda x: abs(mpmath.sin(x)), tan=lambda x: 1 / mpmath.cos(x) ** 2, asin=lambda x: 1 / mpmath.sqrt(1 - x * x),
    acos=lambda x: 1 / mpmath.sqrt(1 - x * x), atan=lambda x: 1 / (1 + x * x), sinh=mpmath.cosh, cosh=lambda x: abs(mpmath.sinh(x)),
    tanh=lambda x: 1 / mpmath.cosh(x) ** 2, erf=lambda x: 2 / mpmath.sqrt(mpmath.pi) * mpmath.exp(-x * x),
    erfc=lambda x: 2 / mpmath.sqrt(mpmath.pi) * mpmath.exp(-x * x), abs=lambda x: mpf(1))
_JUMPS = ('floor', 'ceil', 'step', 'delta')


def _integer_literal(node):
    """n if the exponent node is the literal n or -n with |n| < POWI_LIMIT (the compilers turn x^n into multiplications), else None."""
    sign = 1
    if node[0] == 'neg':
        sign, node = -1, node[1]
    if node[0] == 'num':
        v = mpf(node[1])
        if v == mpmath.floor(v) and v < POWI_LIMIT:
            return sign * int(v)
    return None


class Budget:
    """Rounding allowance of every node in ulps of its value: `exact` for the correctly rounded operations, `functions[name]` (or
    `default`) for sqrt, the transcendentals, 'POW', 'atan2'; x^n with an integer literal n: |n| 2^-52 relative if `powi_counts`
    (repeated multiplication), else that of 'POW'."""

    def __init__(self, default, functions=None, powi_counts=True, exact=0.5):
        self.default, self.functions, self.powi_counts, self.exact = default, dict(functions or {}), powi_counts, exact

    def of(self, name, value, n=None):
        if name in EXACT:
            if name in ('abs', 'neg', 'floor', 'ceil', 'step', 'delta', 'min', 'max', 'select') or mpf(to_double(value)) == value:
                return mpf(0)                       # nothing to round
            return self.exact * ulp(value)
        if name == 'POWI' and self.powi_counts:
            return max(abs(n) * mpf(2) ** -52 * abs(value), self.exact * ulp(value))
        if name == 'POWI':
            name = 'POW'
        return self.functions.get(name, self.default) * ulp(value)


NO_ROUNDING = Budget(0, exact=0)


def _evaluate_one(main, defs, values, budget):
    cache, busy = {}, set()

    def bad(v):
        return mpmath.isnan(v) or mpmath.isinf(v)

    def ev(node):
        kind = node[0]
        if kind == 'num':
            v = mpf(node[1])
            return v, abs(mpf(to_double(v)) - v)             # (a literal reaches the interpreters as the nearest double)
        if kind == 'var':
            name = node[1]
            if name in defs:
                if name not in cache:
                    if name in busy:
                        raise ParseError('circular definition: ' + name)
                    busy.add(name)
                    cache[name] = ev(defs[name])
                    busy.discard(name)
                return cache[name]
            if name == 'random':
                name = 'uniform'
            if name not in values:
                raise ParseError('unknown symbol: ' + name)
            return mpf(values[name]), mpf(0)
        if kind == 'neg':
            v, e = ev(node[1])
            return -v, e
        if kind == 'bin':
            op = node[1]
            (a, ea), (b, eb) = ev(node[2]), ev(node[3])
            if op == '^':
                n = _integer_literal(node[3])
                v = _power(a, b)
                if bad(v) or bad(a) or bad(b):
                    return v, mpf(0)
                if n is not None:
                    slope = abs(n * _power(a, mpf(n - 1))) if n != 0 else mpf(0)
                    return v, slope * ea + budget.of('POWI', v, n)
                e = mpf(0)
                if ea or eb:
                    if a - ea <= 0:
                        raise Unstable('base of a real power may reach zero')
                    for aa in (a - ea, a, a + ea):
                        for bb in (b - eb, b, b + eb):
                            e = max(e, abs(bb * _power(aa, bb - 1)) * ea + abs(_power(aa, bb) * mpmath.log(aa)) * eb)
                return v, e + budget.of('POW', v)
            if bad(a) or bad(b):
                v = _real({'+': lambda: a + b, '-': lambda: a - b, '*': lambda: a * b, '/': lambda: a / b}[op])
                return v, mpf(0)
            if op == '+':
                v, e = a + b, ea + eb
            elif op == '-':
                v, e = a - b, ea + eb
            elif op == '*':
                v, e = a * b, abs(a) * eb + abs(b) * ea + ea * eb
            else:
                if abs(b) <= eb:
                    if eb:
                        raise Unstable('divisor may be zero')
                    return (mpmath.nan if a == 0 else mpmath.inf * (1 if a > 0 else -1)), mpf(0)
                v = a / b
                e = (ea + abs(v) * eb) / (abs(b) - eb)
            return v, e + budget.of(op, v)
        fn, args = node[1], [ev(a) for a in node[2]]
        if fn == 'select':
            (c, ec), yes, no = args
            if ec and abs(c) <= ec:
                raise Unstable('condition of select may be zero')
            return yes if c != 0 else no
        if fn in ('min', 'max'):
            (a, ea), (b, eb) = args
            if mpmath.isnan(a) or mpmath.isnan(b):
                return mpmath.nan, mpf(0)
            return (min(a, b) if fn == 'min' else max(a, b)), max(ea, eb)
        if fn == 'atan2':
            (a, ea), (b, eb) = args
            if bad(a) or bad(b):
                return mpmath.nan, mpf(0)
            v = mpmath.atan2(a, b)
            first = node[2][0]
            if a == 0 and b < 0 and first[0] == 'var' and math.copysign(1.0, values.get(first[1], 0.0)) < 0:
                v = -v                              # atan2(-0, negative) = -pi: the one place where the sign of a zero INPUT decides
            e = mpf(0)
            if ea or eb:
                r = mpmath.sqrt(a * a + b * b) - ea - eb
                if r <= 0 or (b < 0 and abs(a) <= ea):
                    raise Unstable('atan2 at the origin or across its cut')
                e = (abs(b) + eb) / (r * r) * ea + (abs(a) + ea) / (r * r) * eb
            return v, e + budget.of('atan2', v)
        x, ex = args[0]
        if mpmath.isnan(x):
            return mpmath.nan, mpf(0)
        v = _real(_UNARY[fn], x)
        if bad(v):
            return v, mpf(0)
        if fn in _JUMPS:
            if ex and _UNARY[fn](x - ex) != _UNARY[fn](x + ex):
                raise Unstable('%s may jump' % fn)
            return v, budget.of(fn, v)
        e = mpf(0)
        if ex:
            for xx in (x - ex, x, x + ex):
                s = _real(_SLOPE[fn], xx)
                if bad(s) or isinstance(s, mpmath.mpc):
                    raise Unstable('%s leaves its domain' % fn)
                e = max(e, abs(s) * ex)
        return v, e + (budget.of(fn, v) if fn != 'abs' else mpf(0))

    return ev(main)


def evaluate_with_bound(text, values, budget, count=None):
    """[(exact value, error bound of a double evaluation)] per element.  values: {symbol: number or sequence}; 'gaussian' and
    'uniform' are symbols like any other (one value per element, shared by every occurrence)."""
    main, defs = parse(text)
    if count is None:
        lengths = [len(v) for v in values.values() if hasattr(v, '__len__')]
        count = lengths[0] if lengths else 1
    out = []
    with mpmath.workdps(DIGITS):
        for k in range(count):
            row = {name: (float(v[k]) if hasattr(v, '__len__') else float(v)) for name, v in values.items()}
            out.append(_evaluate_one(main, defs, row, budget))
    return out


def evaluate(text, values, count=None):
    """Exact values (mpf at 50 digits; nan where no real value exists) per element."""
    return [v for v, _ in evaluate_with_bound(text, values, NO_ROUNDING, count)]


def mismatches(got, reference):
    """Indices at which a double result lies outside [(value, bound)] of evaluate_with_bound: nan must meet nan, an infinity the same
    infinity, anything else |got - value| <= bound."""
    bad = []
    with mpmath.workdps(DIGITS):
        for k, (g, (v, e)) in enumerate(zip(got, reference)):
            g = float(g)
            if mpmath.isnan(v) or math.isnan(g):
                ok = bool(mpmath.isnan(v)) and math.isnan(g)
            elif math.isinf(to_double(v)) or math.isinf(g):
                ok = to_double(v) == g
            else:
                ok = abs(mpf(g) - v) <= e
            if not ok:
                bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------------------------- corpus
# Grammar corpus: every text uses the symbols of corpus_values() only (x y a b c lambda in (0.2, 0.95), w within 1e-6 of 1, u in
# (-0.95, 0.95), gaussian, uniform), all inside the domain of every function, so that the host paths (math.* raises outside) run them too.
CORPUS = [
    # precedence and associativity
    '-x^2', '2^-x', 'x^-2^2', 'x^y^2', 'a-b-c', 'a/b/c', 'a/b*c', '-a*b', 'a--b', 'a-(b-c)', 'a/(b/c)', '(a+b)*c', 'a+b*c', '-(a+b)', '+a',
    '2*-x', 'a - -b*c', '(-x)^2', '-x^-2', 'a*b^2*c',
    # powers
    'x^2.0', 'x^-2', 'x^(-2)', 'x^0', 'x^1', 'x^0.5', 'w^1048576', 'x^3', 'x^-7', 'u^3', 'u^-2', '(x+y)^(a-b)',
    # number forms
    '1E-3*x', '.5*x', '1.*x', '1e2*x', '2.5e+1*x', '1E8*x', '0.1+0.2*x',
    # names
    'lambda*2', 'lambda^2 + x*lambda',
    # every function once
    'sqrt(x)', 'exp(x)', 'log(x)', 'sin(x)', 'cos(x)', 'tan(x)', 'asin(u)', 'acos(u)', 'atan(u)', 'sinh(u)', 'cosh(u)', 'tanh(u)', 'erf(u)',
    'erfc(u)', 'abs(u)', 'floor(10*u)', 'ceil(10*u)', 'step(u)', 'delta(u-u)', 'delta(u)',
    # operand order
    'select(u-u, a, b)', 'select(x, a, b)', 'select(step(u), b+1, c)', 'min(a, b)', 'max(a, b)', 'min(a, -b)', 'max(-a, b)', 'atan2(a, b)',
    'atan2(u, -b)', 'atan2(-a, u)',
    # definitions: used twice, nested, declared in reverse order
    'k*x + k; k = exp(-a)', 'p*q; p = a+b; q = p*c', 'r + s; s = r*2; r = sqrt(t); t = x+y', 'q^2; p = a*b; q = p+c', 'k; k = -x^2',
    'f*g + f/g; g = 1+y; f = g*x',
    # one draw per evaluation
    'gaussian - gaussian', 'g1 - g2; g1 = gaussian; g2 = gaussian', 'gaussian*x + uniform', 'uniform - k; k = uniform',
    'sqrt(a*(1-z*z))*gaussian + z*u; z = exp(-b*0.5)',
]


def corpus_values(count=50, seed=2024):
    """The corpus inputs: `count` tuples, doubles, the same for every text."""
    import numpy as np
    rng = np.random.default_rng(seed)
    values = {name: rng.uniform(0.2, 0.95, count) for name in ('x', 'y', 'a', 'b', 'c', 'lambda')}
    values['w'] = 1.0 + rng.uniform(-1e-6, 1e-6, count)
    values['u'] = rng.uniform(0.05, 0.95, count) * rng.choice([-1.0, 1.0], count)
    values['gaussian'] = rng.standard_normal(count)
    values['uniform'] = rng.uniform(0.0, 1.0, count)
    return values


# ---------------------------------------------------------------------------------------------------------------- opcode tables
# One short text per opcode over the operands p, q, r, with the inputs at which an implementation goes wrong: signed zeros, the
# smallest normal, +-1, the ends of domains, overflow, arguments near the zeros and poles of the trigonometric functions.
TINY = 2.2250738585072014e-308
_EPS = 2.0 ** -52
_HALF_PI = [k * (math.pi / 2) for k in (1, 2, 3, 4, 10, 63)]
_TRIG = [0.0, -0.0, TINY, 1.0, -1.0, 0.5, 100.0, -100.0, 99.9, 1e-8, 3.0, 22.0, -47.0] + _HALF_PI + [-v for v in _HALF_PI[:3]]
_ROUND = [0.5, -0.5, 1.0, -1.0, -0.0, 0.0, 2.0 ** 52 + 1, 2.5, -2.5, 1e300, -1e300, TINY, -TINY, 0.9999999999999999, -7.000000000000001]
_SIGN = [-0.0, 0.0, TINY, -TINY, 1.0, -1.0, 1e300, -1e-300]
_POWI_BASES = [0.0, 1.0, -1.0, 1.5, -1.5, 0.999, 1.001, -1.001, 2.0, -2.0, 3.0, 1e-3, -0.7, 123.456]
TABLE = {
    'ADD': ('p+q', [(0.1, 0.2), (1.0, -1.0), (1e308, 1e308), (TINY, -TINY), (1.0, 2.0 ** -53), (-0.0, 0.0), (3.5, -1.25), (1e16, 1.0), (-1e308, -1e308)]),
    'SUB': ('p-q', [(3.5, 1.25), (1.25, 3.5), (0.1, 0.3), (1.0, 2.0 ** -53), (0.0, 0.0), (-1e308, 1e308), (1e16, 1.0), (TINY, 0.5 * TINY + TINY)]),
    'MUL': ('p*q', [(0.1, 0.3), (1e200, 1e200), (TINY, 0.5), (-3.0, 7.0), (1.0 + _EPS, 1.0 - _EPS), (1e-200, 1e-200), (-1e200, 1e200), (0.0, -5.0)]),
    'DIV': ('p/q', [(1.0, 3.0), (2.0, -7.0), (1.0, 0.0), (0.0, 0.0), (1e-300, 1e10), (7.0, 2.0), (2.0, 7.0), (-1.0, 0.0), (1e308, 1e-10), (TINY, 3.0)]),
    'NEG': ('-p', [0.0, 1.0, -1.0, TINY, 1e308, -2.5]),
    'abs': ('abs(p)', [0.0, -0.0, 1.0, -1.0, -TINY, -1e308, 2.5]),
    'floor': ('floor(p)', _ROUND),
    'ceil': ('ceil(p)', _ROUND),
    'step': ('step(p)', _SIGN),
    'delta': ('delta(p)', _SIGN),
    'min': ('min(p, q)', [(1.0, 2.0), (2.0, 1.0), (-1.0, -2.0), (-2.0, -1.0), (3.0, 3.0), (-0.0, 0.0), (TINY, -TINY), (1e308, -1e308)]),
    'max': ('max(p, q)', [(1.0, 2.0), (2.0, 1.0), (-1.0, -2.0), (-2.0, -1.0), (3.0, 3.0), (-0.0, 0.0), (TINY, -TINY), (1e308, -1e308)]),
    'select': ('select(p, q, r)', [(1.0, 2.0, 3.0), (0.0, 2.0, 3.0), (-0.0, 2.0, 3.0), (TINY, 2.0, 3.0), (-5.0, 2.0, 3.0), (1e-320, -2.0, -3.0)]),
    'atan2': ('atan2(p, q)', [(1.0, 2.0), (1.0, -2.0), (-1.0, -2.0), (-1.0, 2.0), (2.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0),
                              (0.0, 1.0), (1e300, 1e-300), (1e-300, 1e300), (3.0, -4.0), (-1e-8, -1.0), (0.5, 0.5)]),
    'POW': ('p^q', [(2.0, 0.5), (2.0, -0.5), (10.0, 2.5), (-2.0, 2.0), (-2.0, 3.0), (0.0, 0.0), (-2.0, 0.5), (-8.0, 1.0 / 3), (1.0000001, 1e7),
                    (1e-3, 100.5), (2.0, 1023.5), (2.0, 1024.0), (0.0, 2.0), (0.0, -1.0), (0.3, 0.7), (123.456, -3.21), (1.0, 1e300), (-1.5, -3.0),
                    (0.999, 1e5), (7.0, 1.0), (-3.0, 5.0)]),
    'sqrt': ('sqrt(p)', [0.0, -0.0, TINY, 1.0, 2.0, 0.5, 1e300, 1e-300, 3.0, 4.0, -1.0, 1.0 + _EPS, 1.0 - _EPS / 2, 1.7976931348623157e308]),
    'exp': ('exp(p)', [700.0, -700.0, 0.0, -0.0, TINY, 1.0, -1.0, 0.5, 709.5, -708.0, 710.0, 1e-10, 10.0, -37.5, 0.6931471805599453]),
    'log': ('log(p)', [1.0 + _EPS, 1.0 - _EPS, 1.0 - _EPS / 2, TINY, 1.0, 2.0, 0.5, 10.0, 1e300, 0.0, -1.0, 2.718281828459045, 0.9, 1.1]),
    'sin': ('sin(p)', _TRIG),
    'cos': ('cos(p)', _TRIG),
    'tan': ('tan(p)', _TRIG),
    'asin': ('asin(p)', [1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.999999, 1.0 - _EPS / 2, TINY, 1e-8, 0.7071067811865476, 2.0, -0.3]),
    'acos': ('acos(p)', [1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.999999, 1.0 - _EPS / 2, TINY, 1e-8, 0.7071067811865476, 2.0, -0.3]),
    'atan': ('atan(p)', [0.0, 1.0, -1.0, TINY, 1e300, -1e300, 0.5, 1e-8, 2.414213562373095, -0.4375, 39.0]),
    'sinh': ('sinh(p)', [700.0, -700.0, 0.0, TINY, 1.0, -1.0, 1e-8, 0.5, 20.0, 710.0, -22.0, 0.3]),
    'cosh': ('cosh(p)', [700.0, -700.0, 0.0, TINY, 1.0, -1.0, 1e-8, 0.5, 20.0, 710.0, -22.0, 0.3]),
    'tanh': ('tanh(p)', [20.0, -20.0, 0.0, TINY, 1.0, -1.0, 1e-8, 0.5, 19.06, 0.55, 22.0, -0.3]),
    'erf': ('erf(p)', [0.0, TINY, 1.0, -1.0, 0.5, 1e-8, 2.0, 3.0, 5.9, 6.0, 0.84375, -0.3]),
    'erfc': ('erfc(p)', [5.0, 26.6, 0.0, 1.0, -1.0, 0.5, -5.0, 10.0, 26.0, 30.0, 0.84375, -0.3, 1.25, 2.857, 0.1, 0.25, 0.75,
                           1.5, 1.75, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 6.0, 7.0, 8.0, 9.0, 12.0, 15.0, 18.0, 20.0, 22.0, 25.0, -0.1, -0.75, -2.0, -3.0, 1e-8]),
}
for _n in (0, 1, 2, 3, 7, 64, 1023, -1, -2, -7):
    TABLE['POWI%d' % _n] = ('p^%d' % _n, list(_POWI_BASES))
MEASURED = ('sqrt', 'exp', 'log', 'sin', 'cos', 'tan', 'asin', 'acos', 'atan', 'sinh', 'cosh', 'tanh', 'erf', 'erfc', 'POW', 'atan2')


def table_values(name, count=None):
    """{'p': [...], 'q': [...], 'r': [...]} of TABLE[name], the inputs cycled to `count` elements."""
    rows = [t if isinstance(t, tuple) else (t,) for t in TABLE[name][1]]
    count = count or len(rows)
    rows = [rows[k % len(rows)] for k in range(count)]
    return {sym: [float(row[j]) if j < len(row) else 0.0 for row in rows] for j, sym in enumerate('pqr')}


def _sweep(lo, hi, count=24, log=False):
    """`count` deterministic, unevenly spaced points of (lo, hi) (golden-ratio sequence); log: of 10^(lo..hi)."""
    pts = [lo + (hi - lo) * ((0.5 + k * 0.6180339887498949) % 1.0) for k in range(count)]
    return [10.0 ** v for v in pts] if log else pts


# ordinary arguments next to the edges, so that what is measured per function is its accuracy at large, not at a dozen special points
for _name, _more in dict(
        sqrt=_sweep(-300, 300, log=True), exp=_sweep(-700, 700) + _sweep(-2, 2), log=_sweep(-300, 300, log=True) + _sweep(0.5, 2.0),
        sin=_sweep(-100, 100), cos=_sweep(-100, 100), tan=_sweep(-100, 100), asin=_sweep(-1, 1), acos=_sweep(-1, 1),
        atan=_sweep(-3, 3, log=True) + _sweep(-4, 4), sinh=_sweep(-700, 700) + _sweep(-3, 3), cosh=_sweep(-700, 700) + _sweep(-3, 3),
        tanh=_sweep(-20, 20) + _sweep(-1, 1), erf=_sweep(-6, 6) + _sweep(-1, 1)).items():
    TABLE[_name][1].extend(_more)
TABLE['POW'][1].extend(zip(_sweep(0.2, 5.0), _sweep(-8.0, 8.0)[::-1]))
TABLE['atan2'][1].extend(zip(_sweep(-1.0, 1.0), _sweep(-1.0, 1.0, 25)[1:]))
_cv = corpus_values(66)                              # ... and operand pairs of the corpus' own atan2 texts
TABLE['atan2'][1].extend((float(s), float(t)) for s, t in zip(_cv['a'], _cv['b']))
TABLE['atan2'][1].extend((float(s), -float(t)) for s, t in zip(_cv['u'][:22], _cv['b'][:22]))
TABLE['atan2'][1].extend((-float(s), float(t)) for s, t in zip(_cv['a'][:22], _cv['u'][:22]))
