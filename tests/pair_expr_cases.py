"""TEST INFRASTRUCTURE (checker only) of the pair-expression force (csrc/pair_expr.hip): texts, a reference pair sum and a plain-Python
restatement of the dual-number interpreter.

Reference: a fp64 O(N^2) minimum-image sum over the pairs that are not excluded and have r < rc.  The radial function E(r) and its
derivative come from tests/expr_reference.py -- mpmath at 50 digits, the derivative by mpmath.diff on the same text -- once per
UNIQUE pair of atom types (atoms with equal parameter rows): per type pair they are sampled at Chebyshev nodes of short pieces of
[r_min, rc] (geometric in r, cut at the kinks the text declares) and interpolated in fp64, so that a 1536-atom reference takes
seconds, not the hour that 314 034 evaluations at 50 digits take.  `RadialTable.check` compares the interpolant with mpmath at
radii of its own.  OpenMM's built-in switch S = 1 - 10 t^3 + 15 t^4 - 6 t^5 is applied to (E, E') in closed form.
"""
import math

import mpmath
import numpy as np

import expr_reference as R
from atomsmm_amd import expr as X

KC = 138.935456
SEED = 20241019                                # of the per-type parameter draws
CUTOFF = dict(spcfw=1.0, heaq=0.9)             # cutoffs of the fixtures (q-SPC-FW: L = 2.5; HEAQ-in-water: L = 2.1787)
MIXING = 'chargeprod = charge1*charge2; sigma = 0.5*(sigma1+sigma2); epsilon = sqrt(epsilon1*epsilon2)'

# name -> text, per-particle parameter names, globals, ranges of the per-type parameter draws, kinks(p1, p2, globals) -> radii
TEXTS = {
    'buckingham': dict(text='A*exp(-B*r)-C/r^6; A=sqrt(A1*A2); B=0.5*(B1+B2); C=sqrt(C1*C2)', names=['A', 'B', 'C'], globals={},
                       ranges=dict(A=(2e4, 2e5), B=(28.0, 40.0), C=(1e-3, 6e-3)), kinks=lambda a, b, g: []),
    'wca': dict(text='step(rm-r)*(4*eps*(x^2-x)+eps); x=(sig/r)^6; rm=sig*2^(1/6); sig=0.5*(sig1+sig2); eps=sqrt(eps1*eps2)',
                names=['sig', 'eps'], globals={}, ranges=dict(sig=(0.25, 0.40), eps=(0.2, 1.5)),
                kinks=lambda a, b, g: [0.5 * (a[0] + b[0]) * 2.0 ** (1.0 / 6.0)]),
    'gauss-coulomb': dict(text='Kc*q1*q2*erf(beta*r)/r', names=['q'], globals=dict(Kc=KC, beta=3.5), ranges=dict(q=(0.2, 1.0)),
                          kinks=lambda a, b, g: []),
    'select': dict(text='select(step(sig-r), eps*(1-r/sig)^2, 0) + max(e1,e2)*abs(q1-q2)*exp(-min(r,rcap)/sig); '
                        'sig=0.5*(s1+s2); eps=sqrt(e1*e2)', names=['q', 's', 'e'], globals=dict(rcap=0.8),
                   ranges=dict(q=(-1.0, 1.0), s=(0.3, 0.6), e=(0.5, 2.0)), kinks=lambda a, b, g: [0.5 * (a[1] + b[1]), g['rcap']]),
    'pow': dict(text='eps*(sig/r)^9.5 - C*(r/sig)^(-alpha); sig=0.5*(sig1+sig2); eps=sqrt(eps1*eps2); C=sqrt(C1*C2)',
                names=['sig', 'eps', 'C'], globals=dict(alpha=5.75), ranges=dict(sig=(0.25, 0.40), eps=(0.2, 1.5), C=(0.1, 0.9)),
                kinks=lambda a, b, g: []),
    'morse': dict(text='D*(1-exp(-a*(r-r0)))^2; D=sqrt(D1*D2); a=0.5*(a1+a2); r0=0.5*(r01+r02)', names=['D', 'a', 'r0'], globals={},
                  ranges=dict(D=(1.0, 20.0), a=(8.0, 20.0), r0=(0.25, 0.45)), kinks=lambda a, b, g: []),
}

# (fixture, text) of the GPU comparison against pair_sum: the four texts on both fixtures, and the general power (a non-integer
# and a global exponent: nothing the compiler can fold into multiplications) on the smaller one
GPU_CASES = [(f, t) for f in ('spcfw', 'heaq') for t in ('buckingham', 'wca', 'gauss-coulomb', 'select')] + [('spcfw', 'pow')]


def env_of(case, r, p1, p2, gvalues=None):
    """Symbol values of one pair: r, <name>1, <name>2 and the globals."""
    env = dict(case['globals'] if gvalues is None else gvalues)
    env['r'] = r
    for k, name in enumerate(case['names']):
        env[name + '1'], env[name + '2'] = p1[k], p2[k]
    return env


# ------------------------------------------------------------------------------------------------ the reference radial function
def exact_point(text, env, budget=R.NO_ROUNDING):
    """(E, bound of a double evaluation, dE/dr) at one point: mpmath at 50 digits, the derivative by mpmath.diff on the same text.
    Raises expr_reference.Unstable where the text may jump within rounding."""
    main, defs = R.parse(text)
    with mpmath.workdps(R.DIGITS):
        row = {k: float(v) for k, v in env.items()}
        value, bound = R._evaluate_one(main, defs, row, budget)
        r0 = mpmath.mpf(row['r'])
        slope = mpmath.diff(lambda rr: R._evaluate_one(main, defs, dict(row, r=rr), R.NO_ROUNDING)[0], r0)
    return value, bound, slope


def switch(r, rs, rc):
    """OpenMM's built-in switch and its derivative (fp64 arrays)."""
    t = np.clip((r - rs) / (rc - rs), 0.0, 1.0)
    return 1.0 + t ** 3 * (-10.0 + t * (15.0 - 6.0 * t)), -30.0 * t ** 2 * (1.0 - t) ** 2 / (rc - rs)


class RadialTable:
    """E(r) and E'(r) of one type pair on [lo, hi]: Chebyshev interpolants (fp64) of mpmath values on pieces that grow
    geometrically up to WIDTH and end at every kink.  A piece [a, 1.2 a] keeps the pole of an inverse power at r = 0 eleven
    half-widths from its centre: on the Bernstein ellipse rho = 12, which reaches down to a / 2, r^-13 is 2^13 of its value at a, so
    the Chebyshev error is 2 * 2^13 * 12^-NODES / 11 = 7e-16 of the values on the piece; over a half-width of 0.05 nm, exp(-B r) with
    B = 40 / nm has coefficients I_n(2) ~ 1 / n!: 3e-15 at n = NODES."""
    NODES, RATIO, WIDTH = 17, 1.2, 0.1

    def __init__(self, text, env, lo, hi, kinks=()):
        self.text, self.env = text, dict(env)
        edges = [lo]
        for stop in sorted(k for k in kinks if lo < k < hi) + [hi]:
            while min(edges[-1] * self.RATIO, edges[-1] + self.WIDTH) < stop:
                edges.append(min(edges[-1] * self.RATIO, edges[-1] + self.WIDTH))
            edges.append(stop)
        self.edges = np.array(edges)
        main, defs = R.parse(text)
        nodes = np.cos(np.pi * (np.arange(self.NODES) + 0.5) / self.NODES)
        self.ce, self.cd, self.scale = [], [], []          # per piece: coefficients of E and E', (max |E|, max |E'|) at its nodes
        with mpmath.workdps(R.DIGITS):
            row = {k: float(v) for k, v in self.env.items()}

            def f(rr):
                return R._evaluate_one(main, defs, dict(row, r=rr), R.NO_ROUNDING)[0]
            for a, b in zip(self.edges[:-1], self.edges[1:]):
                rs = [mpmath.mpf(0.5 * (a + b)) + mpmath.mpf(0.5 * (b - a)) * mpmath.mpf(float(t)) for t in nodes]
                e = np.array([float(f(r)) for r in rs])
                d = np.array([float(mpmath.diff(f, r)) for r in rs])
                self.ce.append(np.polynomial.chebyshev.chebfit(nodes, e, self.NODES - 1))
                self.cd.append(np.polynomial.chebyshev.chebfit(nodes, d, self.NODES - 1))
                self.scale.append((max(np.abs(e).max(), 1e-300), max(np.abs(d).max(), 1e-300)))

    def __call__(self, r):
        r = np.asarray(r, dtype=np.float64)
        piece = np.clip(np.searchsorted(self.edges, r, side='right') - 1, 0, len(self.edges) - 2)
        e, d = np.zeros_like(r), np.zeros_like(r)
        for k in np.unique(piece):
            m = piece == k
            a, b = self.edges[k], self.edges[k + 1]
            t = (2.0 * r[m] - (a + b)) / (b - a)
            e[m] = np.polynomial.chebyshev.chebval(t, self.ce[k])
            d[m] = np.polynomial.chebyshev.chebval(t, self.cd[k])
        return e, d

    def check(self, count=12, seed=7):
        """Largest |interpolant - mpmath| of E and of E' at `count` radii of its own, each relative to the largest value at the nodes
        of the piece that holds the radius (what a term of the sum can be off by, in units of its neighbours)."""
        rng = np.random.default_rng(seed)
        rs = rng.uniform(self.edges[0], self.edges[-1], count)
        piece = np.clip(np.searchsorted(self.edges, rs, side='right') - 1, 0, len(self.edges) - 2)
        e, d = self(rs)
        exact = [exact_point(self.text, dict(self.env, r=float(r))) for r in rs]
        ee = np.array([float(v) for v, _, _ in exact])
        dd = np.array([float(s) for _, _, s in exact])
        se = np.array([self.scale[k][0] for k in piece])
        sd = np.array([self.scale[k][1] for k in piece])
        return (np.abs(e - ee) / se).max(), (np.abs(d - dd) / sd).max()


# ------------------------------------------------------------------------------------------------ the pair sum
def pairs_within(positions, box, rc, excl_pairs=()):
    """(i, j, r, unit-free displacement x_i - x_j) of every pair i < j with minimum-image r < rc that is not excluded."""
    pos = np.asarray(positions, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    n = len(pos)
    i, j = np.triu_indices(n, 1)
    d = pos[i] - pos[j]
    d -= box * np.rint(d / box)
    r2 = (d * d).sum(axis=1)
    keep = r2 < rc * rc
    if len(excl_pairs):
        ex = np.sort(np.asarray(excl_pairs, dtype=np.int64).reshape(-1, 2), axis=1)
        ex = ex[ex[:, 0] != ex[:, 1]]
        keep &= ~np.isin(i * n + j, ex[:, 0] * n + ex[:, 1])
    i, j, d = i[keep], j[keep], d[keep]
    return i, j, np.sqrt(r2[keep]), d


DIRECT_BELOW = 100


def pair_terms(case, params, positions, box, rc, excl_pairs=(), gvalues=None, rswitch=None, tables=None):
    """Per-pair (i, j, E, force on i) of the reference, from one RadialTable per unique pair of parameter rows.  `tables`: a dict
    that keeps the tables between calls (same text, globals and cutoff)."""
    params = np.asarray(params, dtype=np.float64).reshape(len(positions), -1)
    g = dict(case['globals'] if gvalues is None else gvalues)
    i, j, r, d = pairs_within(positions, box, rc, excl_pairs)
    rows, kind = np.unique(params, axis=0, return_inverse=True)
    kind = kind.reshape(-1)
    lo_t, hi_t = np.minimum(kind[i], kind[j]), np.maximum(kind[i], kind[j])
    e, de = np.zeros_like(r), np.zeros_like(r)
    tables = {} if tables is None else tables
    for a, b in sorted(set(zip(lo_t.tolist(), hi_t.tolist()))):
        m = (lo_t == a) & (hi_t == b)
        key = (tuple(rows[a]), tuple(rows[b]), tuple(sorted(g.items())), rc)
        if m.sum() < DIRECT_BELOW:          # a handful of pairs (two solute types): mpmath at every one of them
            for k in np.nonzero(m)[0]:
                v, _, slope = exact_point(case['text'], env_of(case, float(r[k]), rows[a], rows[b], g))
                e[k], de[k] = float(v), float(slope)
            continue
        if key not in tables or tables[key].edges[0] > r[m].min():
            tables[key] = RadialTable(case['text'], env_of(case, 1.0, rows[a], rows[b], g), 0.999 * r[m].min(), rc,
                                      case['kinks'](rows[a], rows[b], g))
        e[m], de[m] = tables[key](r[m])
    if rswitch is not None:
        s, ds = switch(r, rswitch, rc)
        e, de = s * e, s * de + ds * e
    f = (-de / r)[:, None] * d
    return i, j, e, f


def pair_sum(case, params, positions, box, rc, excl_pairs=(), gvalues=None, rswitch=None, tables=None, exact=False):
    """(energy, forces [n][3]) of the reference; exact=True accumulates the same terms in mpmath instead of fp64."""
    n = len(positions)
    i, j, e, f = pair_terms(case, params, positions, box, rc, excl_pairs, gvalues, rswitch, tables)
    if not exact:
        forces = np.zeros((n, 3))
        np.add.at(forces, i, f)
        np.add.at(forces, j, -f)
        return float(e.sum()), forces
    with mpmath.workdps(R.DIGITS):
        energy = float(mpmath.fsum(e.tolist()))
        forces = np.zeros((n, 3))
        order = np.argsort(np.concatenate([i, j]), kind='stable')
        who = np.concatenate([i, j])[order]
        what = np.concatenate([f, -f])[order]
        starts = np.searchsorted(who, np.arange(n + 1))
        for a in range(n):
            for c in range(3):
                forces[a, c] = float(mpmath.fsum(what[starts[a]:starts[a + 1], c].tolist()))
    return energy, forces


def typed_parameters(case, type_rows, seed):
    """One parameter row per atom: a draw from case['ranges'] for every unique row of `type_rows` (fixed seed), so that all slots differ
    between atom types and atoms of one type share a row."""
    rng = np.random.default_rng(seed)
    _, kind = np.unique(np.asarray(type_rows, dtype=np.float64).reshape(len(type_rows), -1), axis=0, return_inverse=True)
    kind = kind.reshape(-1)
    table = np.array([[rng.uniform(*case['ranges'][name]) for name in case['names']] for _ in range(kind.max() + 1)])
    return table[kind]


# ------------------------------------------------------------------------------------------------ the interpreter, restated
def _chain(fprime, xd):
    return 0.0 if xd == 0.0 else fprime * xd


def _powi(b, n):
    e, r, q = abs(n), 1.0, b
    while e:
        if e & 1:
            r *= q
        q *= q
        e >>= 1
    return 1.0 / r if n < 0 else r


_FN = dict(exp=lambda x: (math.exp(x),) * 2, log=lambda x: (math.log(x), 1.0 / x), sin=lambda x: (math.sin(x), math.cos(x)),
           cos=lambda x: (math.cos(x), -math.sin(x)), tan=lambda x: (math.tan(x), 1.0 + math.tan(x) ** 2),
           asin=lambda x: (math.asin(x), 1.0 / math.sqrt(1.0 - x * x)), acos=lambda x: (math.acos(x), -1.0 / math.sqrt(1.0 - x * x)),
           atan=lambda x: (math.atan(x), 1.0 / (1.0 + x * x)), sinh=lambda x: (math.sinh(x), math.cosh(x)),
           cosh=lambda x: (math.cosh(x), math.sinh(x)), tanh=lambda x: (math.tanh(x), 1.0 - math.tanh(x) ** 2),
           erf=lambda x: (math.erf(x), 1.1283791670955125739 * math.exp(-(x * x))),
           erfc=lambda x: (math.erfc(x), -(1.1283791670955125739 * math.exp(-(x * x)))))


def run_program(prog, r, p1, p2, gvalues):
    """(E, dE/dr) of a compile_pair program in plain Python: csrc/pair_expr_vm.h word by word -- every slot a (value, d/dr) pair, the
    chain rule through _chain (an operand with derivative exactly zero contributes an exact zero)."""
    names = {v: k for k, v in X.ALL_OPCODES.items()}
    st, loc = [], {}
    for word in prog.code:
        op, arg = names[word & 0xff], word >> 8
        if op == 'CONST':
            st.append((prog.consts[arg], 0.0))
        elif op == 'GLOBAL':
            st.append((float(gvalues[prog.globals_[arg]]), 0.0))
        elif op == 'PAIR_R':
            st.append((r, 1.0))
        elif op == 'PAIR_P1':
            st.append((float(p1[arg]), 0.0))
        elif op == 'PAIR_P2':
            st.append((float(p2[arg]), 0.0))
        elif op == 'LOAD':
            st.append(loc[arg])
        elif op == 'STORE':
            loc[arg] = st.pop()
        elif op in ('ADD', 'SUB', 'MUL', 'DIV', 'POW', 'min', 'max', 'atan2'):
            (b, bd), (a, ad) = st.pop(), st.pop()
            if op == 'ADD':
                st.append((a + b, ad + bd))
            elif op == 'SUB':
                st.append((a - b, ad - bd))
            elif op == 'MUL':
                st.append((a * b, _chain(b, ad) + _chain(a, bd)))
            elif op == 'DIV':
                q = a / b
                st.append((q, 0.0 if ad == 0.0 and bd == 0.0 else (ad - _chain(q, bd)) / b))
            elif op == 'POW':
                v = math.pow(a, b)
                d = _chain(b * math.pow(a, b - 1.0), ad) if ad != 0.0 else 0.0
                if bd != 0.0:
                    d = d + (v * math.log(a)) * bd
                st.append((v, d))
            elif op == 'min':
                st.append((min(a, b), ad if a <= b else bd))
            elif op == 'max':
                st.append((max(a, b), ad if a >= b else bd))
            else:
                st.append((math.atan2(a, b), 0.0 if ad == 0.0 and bd == 0.0 else (b * ad - a * bd) / (b * b + a * a)))
        elif op == 'select':
            (b, bd), (a, ad), (c, _) = st.pop(), st.pop(), st.pop()
            st.append((a, ad) if c != 0.0 else (b, bd))
        elif op == 'NEG':
            v, d = st.pop()
            st.append((-v, -d))
        elif op == 'POWI':
            x, xd = st.pop()
            st.append((_powi(x, arg), 0.0 if arg == 0 else _chain(arg * _powi(x, arg - 1), xd)))
        elif op == 'sqrt':
            x, xd = st.pop()
            v = math.sqrt(x)
            st.append((v, _chain(0.5 / v, xd) if xd != 0.0 else 0.0))
        elif op in _FN:
            x, xd = st.pop()
            v, fp = _FN[op](x)
            st.append((v, _chain(fp, xd)))
        elif op == 'abs':
            x, xd = st.pop()
            st.append((abs(x), xd if x >= 0.0 else -xd))
        elif op in ('floor', 'ceil'):
            x, _ = st.pop()
            st.append((float(math.floor(x) if op == 'floor' else math.ceil(x)), 0.0))
        elif op == 'step':
            x, _ = st.pop()
            st.append((1.0 if x >= 0.0 else 0.0, 0.0))
        elif op == 'delta':
            x, _ = st.pop()
            st.append((1.0 if x == 0.0 else 0.0, 0.0))
        else:
            raise ValueError('not a pair-expression op: ' + op)
    assert len(st) == 1
    return st[0]
