"""Host compiler for CustomIntegrator expressions that are not a kick or a move.

The reference's thermostat / stochastic propagators (src/atomsmm/propagators.py:276-827, 1108-2172) call
`addComputePerDof(variable, expression)`, `addComputeSum(variable, expression)` and `addComputeGlobal(variable,
expression)` with OpenMM's expression syntax: `^` for powers, functions (sqrt, exp, log, sin, ..., step, delta,
select, min, max), and auxiliary definitions after ';' (`vscaling*v; vscaling = exp(-a*dt)`).  Per-DOF and sum
expressions are compiled here into the postfix program that `amm_expr_eval` interprets on the GPU (csrc/expr.hip);
global expressions are evaluated on the host.  `gaussian` / `uniform` are ONE draw per evaluation and degree of
freedom, as in OpenMM (every occurrence inside one expression sees the same value).
"""
import ast
import functools
import keyword
import math
import re

from .utils import InputError

OPCODES = dict(
    CONST=0, GLOBAL=1, BUF=2, MASS=3, GAUSS=4, UNIFORM=5, LOAD=6, STORE=7, DEVG=8, OUT=9,
    ADD=10, SUB=11, MUL=12, DIV=13, NEG=14, POW=15, POWI=16,
    sqrt=20, exp=21, log=22, sin=23, cos=24, tan=25, asin=26, acos=27, atan=28, sinh=29, cosh=30, tanh=31, erf=32,
    erfc=33, abs=34, floor=35, ceil=36, step=37, delta=38, min=39, max=40, select=41, atan2=42, HORNER=43)
# the words only a pair expression has (compile_pair; csrc/pair_expr_vm.h), beside those of OPCODES that it shares
PAIR_OPCODES = dict(PAIR_R=50, PAIR_P1=51, PAIR_P2=52)
# the words only a term expression has (compile_term; csrc/term_expr_vm.h): the term's geometric variable k and its parameter k
TERM_OPCODES = dict(TERM_VAR=53, TERM_P=54)
# the tabulated functions of a pair expression (compile_pair with `functions`; csrc/pair_expr_vm.h): a word's arg is the index of its
# table -- Continuous1DFunction, Discrete1DFunction, Discrete2DFunction
TABLE_OPCODES = dict(TAB_C1=55, TAB_D1=56, TAB_D2=57)
TABLE_KINDS = dict(Continuous1D=('TAB_C1', 1), Discrete1D=('TAB_D1', 1), Discrete2D=('TAB_D2', 2))        # kind -> (word, arguments)
ALL_OPCODES = dict(OPCODES, **PAIR_OPCODES, **TERM_OPCODES, **TABLE_OPCODES)
_ARITY = {'min': 2, 'max': 2, 'select': 3, 'atan2': 2}
MAX_LOCALS = 16
# limits of a pair-expression program (csrc/pair_expr_vm.h)
PAIR_MAX_CODE, PAIR_MAX_CONSTS, PAIR_MAX_GLOBALS, PAIR_MAX_STACK, PAIR_MAX_LOCALS, PAIR_MAX_PARAMS = 256, 48, 48, 16, 16, 3
# a term expression shares them, but for its parameters: one row of doubles per term, not a neighbour row's three (csrc/term_expr_vm.h)
TERM_MAX_PARAMS = 8
PAIR_MAX_TABLES = 8         # tabulated functions of one force (AMM_PEXPR_MAXTABLES)
# a collective-variable expression (compile_cv; csrc/cv.hip): one lane of the outer pass per variable
CV_MAX_CVS, CV_MAX_DERIVS = 16, 16


class ExpressionError(ValueError):
    pass


class NeedsValue(Exception):
    """A deferred global was used where its number is needed (anything but sums and multiples)."""


class Deferred:
    """A global of a host-walked step program whose number waits on device results: const + sum_k coef[k] * slot[k],
    slot[k] being scalars that kernels already enqueued will leave in a device buffer (deriv(energy, lambda) of an AFED
    program, integrators.py:735-737: the extended variable's velocity collects them, nothing else reads it until lambda itself
    moves).  Sums and multiples keep the form, so the host does not wait for the GPU at every deriv(); any other use raises
    NeedsValue and the engine reads the buffer once."""
    __slots__ = ('const', 'terms')

    def __init__(self, const=0.0, terms=None):
        self.const, self.terms = float(const), dict(terms or {})

    def _combined(self, other, sign):
        if isinstance(other, Deferred):
            terms = dict(self.terms)
            for k, c in other.terms.items():
                terms[k] = terms.get(k, 0.0) + sign * c
            return Deferred(self.const + sign * other.const, terms)
        return Deferred(self.const + sign * float(other), self.terms)

    def _scaled(self, factor):
        if isinstance(factor, Deferred):
            raise NeedsValue()
        factor = float(factor)
        return Deferred(self.const * factor, {k: c * factor for k, c in self.terms.items()})

    def __add__(self, other):
        return self._combined(other, 1.0)

    __radd__ = __add__

    def __sub__(self, other):
        return self._combined(other, -1.0)

    def __rsub__(self, other):
        return self._scaled(-1.0)._combined(other, 1.0)

    def __neg__(self):
        return self._scaled(-1.0)

    def __pos__(self):
        return self

    def __mul__(self, other):
        return self._scaled(other)

    __rmul__ = __mul__

    def __truediv__(self, other):
        if isinstance(other, Deferred):
            raise NeedsValue()
        return self._scaled(1.0 / float(other))

    def _needs_value(self, *args):
        raise NeedsValue()

    __rtruediv__ = __pow__ = __rpow__ = __float__ = __abs__ = __bool__ = _needs_value
    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _needs_value
    __hash__ = None

    def resolve(self, values):
        return self.const + sum(c * float(values[k]) for k, c in self.terms.items())


def split_definitions(text):
    """'a*v; a = exp(-g*dt); g = 2' -> ('a*v', {'a': 'exp(-g*dt)', 'g': '2'})."""
    parts = [p.strip() for p in text.split(';') if p.strip()]
    if not parts:
        raise ExpressionError('empty expression')
    defs = {}
    for p in parts[1:]:
        if '=' not in p:
            raise ExpressionError('auxiliary definition without "=": ' + p)
        name, rhs = p.split('=', 1)
        defs[name.strip()] = rhs.strip()
    return parts[0], defs


# legal OpenMM variable names that are Python keywords: lambda (tests/test_systems.py:165), or (the offset radius of the GB texts) ...
_KEYWORD = re.compile(r'\b(%s)\b' % '|'.join(keyword.kwlist))


def _name(node_id):
    return node_id[:-len('__kw')] if node_id.endswith('__kw') else node_id


@functools.lru_cache(maxsize=4096)
def _parse(text):
    """Syntax tree of one expression; cached (a host-walked step program evaluates the same few dozen texts every step;
    nothing that walks the tree modifies it)."""
    try:
        tree = ast.parse(_KEYWORD.sub(r'\1__kw', text).replace('^', '**'), mode='eval').body
        for node in ast.walk(tree):
            if isinstance(node, ast.Name):
                node.id = _name(node.id)
        return tree
    except SyntaxError as exc:
        raise ExpressionError('cannot parse expression %r: %s' % (text, exc))


class Program:
    """Postfix program for amm_expr_eval: `code` (opcode | arg << 8), `consts`, and the names of the global values the
    launch must supply, in order (`globals_`)."""

    def __init__(self):
        self.code, self.consts, self.globals_ = [], [], []

    def emit(self, op, arg=0):
        self.code.append(ALL_OPCODES[op] | (int(arg) << 8))

    def const(self, value):
        value = float(value)
        for k, c in enumerate(self.consts):
            if c == value and math.copysign(1.0, c) == math.copysign(1.0, value):
                return k
        self.consts.append(value)
        return len(self.consts) - 1

    def global_index(self, name):
        if name not in self.globals_:
            self.globals_.append(name)
        return self.globals_.index(name)


def _folded_trees(main, defs):
    """Syntax trees of the main expression and of the definitions with every subexpression of literals -- and of definitions that
    come down to a literal, `b = 2.5` -- replaced by its value in double arithmetic (what Lepton's optimiser does to a
    CustomNonbondedForce text): the coefficients of a force-switched potential are polynomials in such a `b`.  New nodes: the cached
    trees of _parse are not touched."""
    memo, busy = {}, set()

    def definition(name):
        if name not in memo:
            if name in busy:
                raise ExpressionError('circular auxiliary definition: ' + name)
            busy.add(name)
            memo[name] = fold(_parse(defs[name]))
            busy.discard(name)
        return memo[name]

    def number(node):
        return isinstance(node, ast.Constant) and isinstance(node.value, (int, float))

    def fold(node):
        if isinstance(node, ast.Name):
            if node.id in defs:
                tree = definition(node.id)
                return tree if number(tree) else node
            return node
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            operand = fold(node.operand)
            if number(operand):
                return ast.Constant(value=-float(operand.value) if isinstance(node.op, ast.USub) else float(operand.value))
            return ast.UnaryOp(op=node.op, operand=operand)
        if isinstance(node, ast.BinOp):
            left, right = fold(node.left), fold(node.right)
            if number(left) and number(right):
                a, b = float(left.value), float(right.value)
                try:
                    if isinstance(node.op, ast.Pow) and b == int(b) and abs(b) < 1 << 20:
                        q, value, e = a, 1.0, abs(int(b))          # as the interpreters take an integer power
                        while e:
                            if e & 1:
                                value *= q
                            q *= q
                            e >>= 1
                        value = 1.0 / value if b < 0 else value
                    else:
                        value = {ast.Add: lambda: a + b, ast.Sub: lambda: a - b, ast.Mult: lambda: a * b, ast.Div: lambda: a / b,
                                 ast.Pow: lambda: math.pow(a, b)}[type(node.op)]()
                    return ast.Constant(value=float(value))
                except (KeyError, ArithmeticError, ValueError):
                    pass               # (left to the device, which has an answer for 1/0)
            return ast.BinOp(left=left, op=node.op, right=right)
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and not node.keywords:
            args = [fold(a) for a in node.args]
            if node.func.id in _HOST_FUNCS and len(args) == _ARITY.get(node.func.id, 1) and all(number(a) for a in args):
                try:
                    return ast.Constant(value=float(_HOST_FUNCS[node.func.id](*[float(a.value) for a in args])))
                except (ArithmeticError, ValueError):
                    pass
            return ast.Call(func=node.func, args=args, keywords=[])
        return node

    return fold(_parse(main)), definition


def compile_per_dof(text, resolve, what='per-DOF', random_ok=True, fold=False, functions=None, name_calls=None):
    """Compile a per-DOF (or sum) expression.  `resolve(name)` returns ('buf', slot), ('mass',), ('global',), ('op', opcode name, arg)
    or None.  `what` names the kind of expression in error messages; random_ok=False: `gaussian` / `uniform` are errors; fold=True:
    subexpressions of literals are evaluated here (_folded_trees); functions: name -> (word, arguments, index) of the tabulated
    functions a call may name (compile_pair only); name_calls(fn, args): for a call whose arguments are names, not expressions
    (distance(p1,p2) of compile_compound) -- the syntax nodes of the arguments in, ('op', opcode name, arg) out, or None when `fn`
    is no such function."""
    main, defs = split_definitions(text)
    prog = Program()
    local_of, in_progress = {}, set()
    main_tree, tree_of = (_folded_trees(main, defs) if fold else (_parse(main), lambda name: _parse(defs[name])))

    def gen(node):
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            prog.emit('CONST', prog.const(node.value))
        elif isinstance(node, ast.Name):
            name = node.id
            if name in defs and fold and isinstance(tree_of(name), ast.Constant):
                prog.emit('CONST', prog.const(tree_of(name).value))
            elif name in defs:
                if name not in local_of:
                    if name in in_progress:
                        raise ExpressionError('circular auxiliary definition: ' + name)
                    if len(local_of) + len(in_progress) >= MAX_LOCALS:
                        raise ExpressionError('too many auxiliary definitions')
                    in_progress.add(name)
                    gen(tree_of(name))
                    in_progress.discard(name)
                    local_of[name] = len(local_of)
                    prog.emit('STORE', local_of[name])
                prog.emit('LOAD', local_of[name])
            elif name in ('gaussian', 'uniform', 'random') and not random_ok:
                raise ExpressionError('random numbers (%s) are not defined in a %s expression' % (name, what))
            elif name == 'gaussian':
                prog.emit('GAUSS')
            elif name in ('uniform', 'random'):
                prog.emit('UNIFORM')
            else:
                kind = resolve(name)
                if kind is None:
                    raise ExpressionError('unknown symbol in %s expression: %s' % (what, name))
                if kind[0] == 'op':
                    prog.emit(kind[1], kind[2])
                elif kind[0] == 'buf':
                    prog.emit('BUF', kind[1])
                elif kind[0] == 'mass':
                    prog.emit('MASS')
                else:
                    prog.emit('GLOBAL', prog.global_index(name))
        elif isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            gen(node.operand)
            if isinstance(node.op, ast.USub):
                prog.emit('NEG')
        elif isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div, ast.Pow)):
            if isinstance(node.op, ast.Pow):
                e = node.right
                neg = isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub)
                ev = e.operand if neg else e
                if isinstance(ev, ast.Constant) and float(ev.value) == int(ev.value) and abs(int(ev.value)) < 1 << 20:
                    gen(node.left)
                    prog.emit('POWI', -int(ev.value) if neg else int(ev.value))
                    return
            gen(node.left)
            gen(node.right)
            prog.emit({ast.Add: 'ADD', ast.Sub: 'SUB', ast.Mult: 'MUL', ast.Div: 'DIV', ast.Pow: 'POW'}[type(node.op)])
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and not node.keywords:
            fn = node.func.id
            special = name_calls(fn, node.args) if name_calls else None
            if special is not None:
                prog.emit(special[1], special[2])
                return
            if functions and fn in functions:
                word, arity, index = functions[fn]
                if len(node.args) != arity:
                    raise ExpressionError('tabulated function %s takes %d argument%s (%d given)' % (fn, arity, '' if arity == 1 else 's', len(node.args)))
                for a in node.args:
                    gen(a)
                prog.emit(word, index)
                return
            if fn not in OPCODES or fn.isupper() or len(node.args) != _ARITY.get(fn, 1):
                raise ExpressionError('unsupported function call: %s/%d' % (fn, len(node.args)))
            for a in node.args:
                gen(a)
            prog.emit(fn)
        else:
            raise ExpressionError('unsupported syntax in expression: ' + ast.dump(node))

    gen(main_tree)
    return prog


_STACK_EFFECT = {'CONST': 1, 'GLOBAL': 1, 'PAIR_R': 1, 'PAIR_P1': 1, 'PAIR_P2': 1, 'TERM_VAR': 1, 'TERM_P': 1, 'LOAD': 1, 'STORE': -1, 'ADD': -1, 'SUB': -1, 'MUL': -1,
                 'DIV': -1, 'POW': -1, 'min': -1, 'max': -1, 'atan2': -1, 'select': -2, 'TAB_C1': 0, 'TAB_D1': 0, 'TAB_D2': -1}


def compile_pair(text, per_particle_names, global_names, functions=None):
    """Compile the energy text of a CustomNonbondedForce for the pair-expression kernel (csrc/pair_expr.hip): `r` is PAIR_R, the row
    atom's parameter `<name>1` is PAIR_P1 k and the neighbour's `<name>2` PAIR_P2 k (k: position in per_particle_names), a global
    parameter GLOBAL k (k: position in the program's globals_); auxiliary definitions, in any order, become locals.  functions: the
    force's tabulated functions, name -> (kind of TABLE_KINDS, arguments) in the force's order -- a call of one compiles its arguments,
    then the kind's word TAB_* with the function's index.  The limits of csrc/pair_expr_vm.h are enforced here, each with an
    ExpressionError that names it."""
    per_particle_names, global_names = list(per_particle_names), set(global_names)
    if len(per_particle_names) > PAIR_MAX_PARAMS:
        raise ExpressionError('a pair expression takes at most %d per-particle parameters (%d given)' % (PAIR_MAX_PARAMS, len(per_particle_names)))
    slots = {}
    for k, name in enumerate(per_particle_names):
        slots[name + '1'] = ('op', 'PAIR_P1', k)
        slots[name + '2'] = ('op', 'PAIR_P2', k)

    def resolve(name):
        if name == 'r':
            return ('op', 'PAIR_R', 0)
        if name in slots:
            return slots[name]
        return ('global',) if name in global_names else None

    words = None
    if functions:
        if len(functions) > PAIR_MAX_TABLES:
            raise ExpressionError('a pair expression takes at most %d tabulated functions (%d given)' % (PAIR_MAX_TABLES, len(functions)))
        words = {}
        for index, (name, (kind, arity)) in enumerate(functions.items()):
            if kind not in TABLE_KINDS:
                raise ExpressionError('tabulated function %s: kind %s is not one a pair expression evaluates' % (name, kind))
            if arity != TABLE_KINDS[kind][1]:
                raise ExpressionError('tabulated function %s: a %sFunction takes %d argument%s (%d declared)' %
                                      (name, kind, TABLE_KINDS[kind][1], '' if TABLE_KINDS[kind][1] == 1 else 's', arity))
            if name in _HOST_FUNCS:
                raise ExpressionError('tabulated function %s shadows the built-in function of that name' % name)
            if name == 'r' or name in slots or name in per_particle_names or name in global_names:
                raise ExpressionError('tabulated function %s shadows %s' % (name, 'the distance r' if name == 'r' else 'the parameter of that name'))
            words[name] = (TABLE_KINDS[kind][0], arity, index)
    return _checked_program(text, resolve, 'pair', words)


def table_words(code):
    """The (word name, table index) of every tabulated-function word of a program's code, in order."""
    names = {v: k for k, v in TABLE_OPCODES.items()}
    return [(names[w & 0xff], w >> 8) for w in code if (w & 0xff) in names]


def _checked_program(text, resolve, what, functions=None, name_calls=None):
    """The folded program of a pair or term energy text, held against the limits of csrc/pair_expr_vm.h."""
    try:
        prog = compile_per_dof(text, resolve, what=what, random_ok=False, fold=True, functions=functions, name_calls=name_calls)
    except ExpressionError as exc:
        if 'too many auxiliary definitions' in str(exc):
            raise ExpressionError('%s expression: more than %d auxiliary definitions (locals)' % (what, PAIR_MAX_LOCALS))
        raise
    if len(prog.code) > PAIR_MAX_CODE:
        raise ExpressionError('%s expression: %d code words (limit %d)' % (what, len(prog.code), PAIR_MAX_CODE))
    if len(prog.consts) > PAIR_MAX_CONSTS:
        raise ExpressionError('%s expression: %d constants (limit %d)' % (what, len(prog.consts), PAIR_MAX_CONSTS))
    if len(prog.globals_) > PAIR_MAX_GLOBALS:
        raise ExpressionError('%s expression: %d global parameters (limit %d)' % (what, len(prog.globals_), PAIR_MAX_GLOBALS))
    names = {v: k for k, v in ALL_OPCODES.items()}
    depth = deepest = 0
    for word in prog.code:
        depth += _STACK_EFFECT.get(names[word & 0xff], 0)
        deepest = max(deepest, depth)
    if deepest > PAIR_MAX_STACK:
        raise ExpressionError('%s expression: stack depth %d (limit %d)' % (what, deepest, PAIR_MAX_STACK))
    return prog


def compile_term(text, variables, per_term_names, global_names, what='term'):
    """Compile the energy text of a CustomBondForce / CustomAngleForce / CustomTorsionForce / CustomExternalForce for the
    term-expression kernels (csrc/term_expr.hip): variable k of `variables` -- ('r',), ('theta',) or ('x', 'y', 'z') -- is TERM_VAR k,
    per-term parameter k TERM_P k, a global parameter GLOBAL k (k: position in the program's globals_); auxiliary definitions, in any
    order, become locals.  The limits are those of compile_pair, but for the parameters: up to TERM_MAX_PARAMS per term."""
    variables, per_term_names, global_names = list(variables), list(per_term_names), set(global_names)
    if len(per_term_names) > TERM_MAX_PARAMS:
        raise InputError('a term expression takes at most %d per-term parameters (%d given)' % (TERM_MAX_PARAMS, len(per_term_names)))
    if re.search(r'\bperiodicdistance\s*\(', text):
        raise ExpressionError('periodicdistance(...) is not supported in a term expression')

    def resolve(name):
        if name in per_term_names:
            return ('op', 'TERM_P', per_term_names.index(name))
        if name in variables:
            return ('op', 'TERM_VAR', variables.index(name))
        return ('global',) if name in global_names else None

    return _checked_program(text, resolve, what)


# a compound-bond expression (compile_compound; csrc/compound.hip): particles (or groups) of a bond, geometric variables of a text
COMPOUND_MAX_SLOTS, COMPOUND_MAX_VARS = 8, 16
_COMPOUND_CALLS = dict(distance=2, angle=3, dihedral=4)          # function -> particles it takes
_COMPOUND_REFUSED = ('pointdistance', 'pointangle', 'pointdihedral')


def compile_compound(text, n_slots, prefix, per_bond_names, global_names):
    """Compile the energy text of a CustomCompoundBondForce (prefix 'p') or CustomCentroidBondForce (prefix 'g') for the compound-bond
    kernel (csrc/compound.hip).  Returns (program, variables): variables[k] = (kind, slots) is what TERM_VAR k reads -- kind 'x', 'y'
    or 'z' (the raw coordinate <kind><slot + 1>), 'distance', 'angle' or 'dihedral' (a call whose arguments are bare particle names
    <prefix>1 .. <prefix>N), slots the 0-based positions within the bond -- in the order of first use; identical calls share one
    variable.  Per-bond parameter k is TERM_P k, a global parameter GLOBAL k; auxiliary definitions become locals.  The limits are
    those of compile_term plus COMPOUND_MAX_SLOTS and COMPOUND_MAX_VARS, each an error that names it."""
    per_bond_names, global_names = list(per_bond_names), set(global_names)
    what = 'compound-bond'
    unit_ = 'groups' if prefix == 'g' else 'particles'
    if not 1 <= int(n_slots) <= COMPOUND_MAX_SLOTS:
        raise InputError('a %s expression takes 1 to %d %s per bond (%d given)' % (what, COMPOUND_MAX_SLOTS, unit_, n_slots))
    if len(per_bond_names) > TERM_MAX_PARAMS:
        raise InputError('a %s expression takes at most %d per-bond parameters (%d given)' % (what, TERM_MAX_PARAMS, len(per_bond_names)))
    if re.search(r'\bperiodicdistance\s*\(', text):
        raise ExpressionError('periodicdistance(...) is not supported in a %s expression' % what)
    particles = {'%s%d' % (prefix, k + 1): k for k in range(int(n_slots))}
    coordinates = {'%s%d' % (axis, k + 1): (axis, (k,)) for axis in 'xyz' for k in range(int(n_slots))}
    return _geometric_program(text, what, unit_, 'a bond (%s1 .. %s%d)' % (prefix, prefix, n_slots), '%s1 .. %s%d' % (prefix, prefix, n_slots),
                              particles, coordinates, per_bond_names, global_names)


def _geometric_program(text, what, unit_, owner, names_hint, particles, coordinates, parameter_names, global_names, refused_names=None):
    """The body compile_compound and compile_hbond share.  particles: name -> slot of the names that stand as arguments of distance /
    angle / dihedral; coordinates: name -> (axis, (slot,)) of the raw coordinates the text may read; parameter k of parameter_names is
    TERM_P k; refused_names(name): raises for a name the kind of text refuses, else returns None.  Returns (program, variables)."""
    for name in parameter_names + sorted(global_names):
        if name in particles or name in coordinates:
            raise ExpressionError('%s expression: the parameter %s shadows the %s of that name' % (
                what, name, 'coordinate' if name in coordinates else unit_[:-1]))
    variables = []

    def variable(entry):
        if entry not in variables:
            if len(variables) >= COMPOUND_MAX_VARS:
                raise ExpressionError('%s expression: more than %d distinct geometric variables' % (what, COMPOUND_MAX_VARS))
            variables.append(entry)
        return ('op', 'TERM_VAR', variables.index(entry))

    def resolve(name):
        if name in parameter_names:
            return ('op', 'TERM_P', parameter_names.index(name))
        if name in coordinates:
            return variable(coordinates[name])
        if name in particles:
            raise ExpressionError('%s expression: %s names one of the %s; it stands only as an argument of distance, angle or dihedral' % (what, name, unit_))
        if name in global_names:
            return ('global',)
        if refused_names is not None:
            refused_names(name)
        return None

    def name_calls(fn, args):
        if fn in _COMPOUND_REFUSED:
            raise ExpressionError('%s(...) is not supported in a %s expression' % (fn, what))
        if fn not in _COMPOUND_CALLS:
            return None
        if len(args) != _COMPOUND_CALLS[fn]:
            raise ExpressionError('%s takes %d %s (%d given)' % (fn, _COMPOUND_CALLS[fn], unit_, len(args)))
        slots = []
        for a in args:
            if not isinstance(a, ast.Name):
                raise ExpressionError('%s expression: the arguments of %s are bare names of %s (%s), not expressions' % (
                    what, fn, unit_, names_hint))
            if a.id not in particles:
                raise ExpressionError('%s expression: %s is none of the %s of %s' % (what, a.id, unit_, owner))
            slots.append(particles[a.id])
        return variable((fn, tuple(slots)))

    return _checked_program(text, resolve, what, name_calls=name_calls), variables


HBOND_SLOTS = dict(d1=0, d2=1, d3=2, a1=3, a2=4, a3=5)      # the six particles of a donor-acceptor pair


def compile_hbond(text, per_donor_names, per_acceptor_names, global_names):
    """Compile the energy text of a CustomHbondForce for the hydrogen-bond kernel (csrc/hbond.hip).  Returns (program, variables) as
    compile_compound does: variables[k] = (kind, slots), kind 'distance', 'angle' or 'dihedral' over the bare names d1 d2 d3 a1 a2 a3
    = slots 0 .. 5, in the order of first use, identical calls sharing one variable.  Per-donor parameter k is TERM_P k, the
    per-acceptor parameters follow the per-donor ones; a global parameter is GLOBAL k.  The class has no coordinate variables: x1 ...
    are refused by name, as are pointdistance and its kin and periodicdistance.  The limits are TERM_MAX_PARAMS parameters (donors' and
    acceptors' together) and COMPOUND_MAX_VARS variables, each an error that names it."""
    per_donor_names, per_acceptor_names, global_names = list(per_donor_names), list(per_acceptor_names), set(global_names)
    what = 'hydrogen-bond'
    names = per_donor_names + per_acceptor_names
    if len(names) > TERM_MAX_PARAMS:
        raise InputError('a %s expression takes at most %d per-donor and per-acceptor parameters together (%d + %d given)' % (
            what, TERM_MAX_PARAMS, len(per_donor_names), len(per_acceptor_names)))
    for name in names:
        if names.count(name) > 1:
            raise ExpressionError('%s expression: the parameter %s is declared twice among the per-donor and per-acceptor parameters' % (what, name))
    if re.search(r'\bperiodicdistance\s*\(', text):
        raise ExpressionError('periodicdistance(...) is not supported in a %s expression' % what)

    def refused_names(name):
        if re.fullmatch(r'[xyz][0-9]+', name):
            raise ExpressionError('%s expression: the raw coordinate %s is not supported (a CustomHbondForce text reads distance, angle and '
                                  'dihedral of d1 d2 d3 a1 a2 a3 only)' % (what, name))

    return _geometric_program(text, what, 'particles', 'a donor-acceptor pair (d1 d2 d3 a1 a2 a3)', 'd1 d2 d3 a1 a2 a3', dict(HBOND_SLOTS), {},
                              names, global_names, refused_names)


MANY_PARTICLE_MAX_PARAMS = 2     # per-particle parameters of a many-particle text: three suffixed copies each


def many_particle_parameter_names(n_slots, per_particle_names):
    """The names a many-particle text reads its per-particle parameters by, in the order of TERM_P: role by role (sigma1, eps1,
    sigma2, eps2, sigma3, eps3)."""
    return ['%s%d' % (name, r + 1) for r in range(int(n_slots)) for name in per_particle_names]


def compile_many_particle(text, n_slots, per_particle_names, global_names):
    """Compile the energy text of a CustomManyParticleForce for the many-particle kernel (csrc/manyparticle.hip).  Returns (program,
    variables) as compile_compound does: variables[k] = (kind, slots), kind 'distance', 'angle' or 'dihedral' over the bare names
    p1 .. p<n_slots>, or 'x', 'y', 'z' for the raw coordinates x1 .. z<n_slots> (never wrapped), in the order of first use,
    identical calls sharing one variable.  Per-particle parameter k of the particle in role r (named <name><r + 1>) is TERM_P
    r * P + k; a global parameter is GLOBAL k.  pointdistance and its kin and periodicdistance are refused by name.  The limits are
    MANY_PARTICLE_MAX_PARAMS per-particle parameters (n_slots * P <= TERM_MAX_PARAMS) and COMPOUND_MAX_VARS variables, each an error
    that names it."""
    per_particle_names, global_names = list(per_particle_names), set(global_names)
    what = 'many-particle'
    n_slots = int(n_slots)
    if not 1 <= n_slots <= COMPOUND_MAX_SLOTS:
        raise InputError('a %s expression takes 1 to %d particles per set (%d given)' % (what, COMPOUND_MAX_SLOTS, n_slots))
    if len(per_particle_names) > MANY_PARTICLE_MAX_PARAMS or n_slots * len(per_particle_names) > TERM_MAX_PARAMS:
        raise InputError('a %s expression takes at most %d per-particle parameters (%d given; each has %d suffixed copies, at most %d '
                         'together)' % (what, MANY_PARTICLE_MAX_PARAMS, len(per_particle_names), n_slots, TERM_MAX_PARAMS))
    for name in per_particle_names:
        if per_particle_names.count(name) > 1:
            raise ExpressionError('%s expression: the per-particle parameter %s is declared twice' % (what, name))
    if re.search(r'\bperiodicdistance\s*\(', text):
        raise ExpressionError('periodicdistance(...) is not supported in a %s expression' % what)
    particles = {'p%d' % (k + 1): k for k in range(n_slots)}
    coordinates = {'%s%d' % (axis, k + 1): (axis, (k,)) for axis in 'xyz' for k in range(n_slots)}
    hint = 'p1 .. p%d' % n_slots

    def refused_names(name):
        if name in per_particle_names:
            raise ExpressionError('%s expression: the per-particle parameter %s is read with the suffix of its particle (%s1 .. %s%d)' % (
                what, name, name, name, n_slots))

    return _geometric_program(text, what, 'particles', 'a set (%s)' % hint, hint, particles, coordinates,
                              many_particle_parameter_names(n_slots, per_particle_names), global_names, refused_names)


def compile_cv(text, cv_names, deriv_names, global_names):
    """Compile the energy text of a CustomCVForce for the collective-variable kernel (csrc/cv.hip): collective variable k of `cv_names`
    is TERM_VAR k, and the parameters the force asked derivatives for (`deriv_names`) follow as TERM_VAR K + p -- variables, not
    globals, so that the kernel can seed each of them; every other parameter is GLOBAL k.  compile_term without per-term
    parameters; the limits are its own plus CV_MAX_CVS and CV_MAX_DERIVS."""
    cv_names, deriv_names = list(cv_names), list(deriv_names)
    what = 'collective-variable'
    if len(cv_names) > CV_MAX_CVS:
        raise ExpressionError('%s expression: %d collective variables (limit %d)' % (what, len(cv_names), CV_MAX_CVS))
    if len(deriv_names) > CV_MAX_DERIVS:
        raise ExpressionError('%s expression: %d energy parameter derivatives (limit %d)' % (what, len(deriv_names), CV_MAX_DERIVS))
    if len(set(cv_names + deriv_names)) != len(cv_names) + len(deriv_names):
        raise ExpressionError('%s expression: a name is used twice among the collective variables and the derivative parameters' % what)
    return compile_term(text, cv_names + deriv_names, [], set(global_names) - set(deriv_names), what=what)


# a custom generalized-Born force (compile_custom_gb; csrc/custom_gb.hip): computed values, energy terms and their types
CGB_MAX_VALUES, CGB_MAX_TERMS = 4, 8
CGB_SINGLE, CGB_PAIR, CGB_PAIR_NOEXCL = 0, 1, 2          # CustomGBForce.SingleParticle / ParticlePair / ParticlePairNoExclusions
CGB_VAR_V1, CGB_VAR_V2, CGB_P2 = 1, 5, 8                 # TERM_VAR 0 is r, 1 + k / 5 + k value k of particle 1 / 2; TERM_P 8 + k parameter k of particle 2


class CustomGBPrograms:
    """What compile_custom_gb returns: `values` and `terms` (one Program each, in the force's order), `types` (the values', then the
    terms'), `value_reads[m]` / `term_reads[t]` (the indices of the computed values that the text reads of particle 1 -- of the
    particle itself in a single-particle text: what the kernels differentiate it in), and `globals_`, the force's global parameters
    in ITS order: GLOBAL k of every program is entry k of this one list."""

    def __init__(self, values, terms, types, value_reads, term_reads, globals_):
        self.values, self.terms, self.types = values, terms, types
        self.value_reads, self.term_reads, self.globals_ = value_reads, term_reads, globals_

    @property
    def programs(self):
        return self.values + self.terms


def compile_custom_gb(per_particle_names, global_names, values, terms, functions=None):
    """Compile a CustomGBForce for the kernels of csrc/custom_gb.hip.  values: [(name, text, type)] of addComputedValue; terms:
    [(text, type)] of addEnergyTerm; functions: as for compile_pair.  In a pair text `r` is TERM_VAR 0, `<parameter>1` / `<parameter>2`
    TERM_P k / TERM_P 8 + k and `<value>1` / `<value>2` TERM_VAR 1 + k / 5 + k; in a single-particle text the bare names are TERM_P k
    and TERM_VAR 1 + k.  A computed value sees the values before it (a pair-type value, legal in first place only, none); an energy
    term sees all.  A global parameter is GLOBAL k, k its position among the force's globals.  The limits are those of
    csrc/pair_expr_vm.h per program plus TERM_MAX_PARAMS parameters, CGB_MAX_VALUES values, CGB_MAX_TERMS terms and PAIR_MAX_TABLES
    functions, each an ExpressionError that names it."""
    what = 'custom-GB'
    pnames, gnames = list(per_particle_names), list(global_names)
    values, terms = [tuple(v) for v in values], [tuple(t) for t in terms]
    vnames = [v[0] for v in values]
    if len(pnames) > TERM_MAX_PARAMS:
        raise ExpressionError('a %s force takes at most %d per-particle parameters (%d given)' % (what, TERM_MAX_PARAMS, len(pnames)))
    if len(values) > CGB_MAX_VALUES:
        raise ExpressionError('a %s force takes at most %d computed values (%d given)' % (what, CGB_MAX_VALUES, len(values)))
    if len(terms) > CGB_MAX_TERMS:
        raise ExpressionError('a %s force takes at most %d energy terms (%d given)' % (what, CGB_MAX_TERMS, len(terms)))
    if len(gnames) > PAIR_MAX_GLOBALS:
        raise ExpressionError('a %s force takes at most %d global parameters (%d given)' % (what, PAIR_MAX_GLOBALS, len(gnames)))
    functions = dict(functions or {})
    if len(functions) > PAIR_MAX_TABLES:
        raise ExpressionError('a %s force takes at most %d tabulated functions (%d given)' % (what, PAIR_MAX_TABLES, len(functions)))
    declared = pnames + vnames + gnames + list(functions)
    for name in declared:
        if declared.count(name) > 1:
            raise ExpressionError('%s force: the name %s is used twice among the per-particle parameters, computed values, global '
                                  'parameters and tabulated functions' % (what, name))
        if name == 'r' or name in _HOST_FUNCS:
            raise ExpressionError('%s force: the name %s shadows %s' % (what, name, 'the distance r' if name == 'r' else 'the built-in function of that name'))
    words = {}
    for index, (name, (kind, arity)) in enumerate(functions.items()):
        if kind not in TABLE_KINDS:
            raise ExpressionError('tabulated function %s: kind %s is not one a %s expression evaluates' % (name, kind, what))
        if arity != TABLE_KINDS[kind][1]:
            raise ExpressionError('tabulated function %s: a %sFunction takes %d argument%s (%d declared)' %
                                  (name, kind, TABLE_KINDS[kind][1], '' if TABLE_KINDS[kind][1] == 1 else 's', arity))
        words[name] = (TABLE_KINDS[kind][0], arity, index)
    types = [int(v[2]) for v in values] + [int(t[1]) for t in terms]
    for kind in types:
        if kind not in (CGB_SINGLE, CGB_PAIR, CGB_PAIR_NOEXCL):
            raise ExpressionError('%s force: unknown computation type %r' % (what, kind))
    for place, (name, _, kind) in enumerate(values):
        if place > 0 and int(kind) != CGB_SINGLE:
            raise ExpressionError('%s force: the computed value %s is a sum over pairs in place %d; only the first computed value may be '
                                  'of a pair type' % (what, name, place))

    def one(text, kind, visible, label):
        """The program of one text that sees the first `visible` computed values."""
        coordinates = sorted(symbols(text) & {'x', 'y', 'z'} - set(declared))
        if coordinates:
            raise ExpressionError('%s: the particle coordinate %s in a text is not supported (a %s text reads r, parameters, computed '
                                  'values and global parameters)' % (label, coordinates[0], what))
        slots = {}
        if kind == CGB_SINGLE:
            for k, name in enumerate(pnames):
                slots[name] = ('op', 'TERM_P', k)
            for k, name in enumerate(vnames[:visible]):
                slots[name] = ('op', 'TERM_VAR', CGB_VAR_V1 + k)
        else:
            slots['r'] = ('op', 'TERM_VAR', 0)
            for k, name in enumerate(pnames):
                slots[name + '1'] = ('op', 'TERM_P', k)
                slots[name + '2'] = ('op', 'TERM_P', CGB_P2 + k)
            for k, name in enumerate(vnames[:visible]):
                slots[name + '1'] = ('op', 'TERM_VAR', CGB_VAR_V1 + k)
                slots[name + '2'] = ('op', 'TERM_VAR', CGB_VAR_V2 + k)

        def resolve(name):
            if name in slots:
                return slots[name]
            return ('global',) if name in gnames else None

        try:
            prog = _checked_program(text, resolve, what, words or None)
        except ExpressionError as exc:
            raise ExpressionError('%s: %s' % (label, exc))
        # GLOBAL k: from the program's own order of first use to the force's order
        for pc, word in enumerate(prog.code):
            if word & 0xff == OPCODES['GLOBAL']:
                prog.code[pc] = OPCODES['GLOBAL'] | (gnames.index(prog.globals_[word >> 8]) << 8)
        prog.globals_ = list(gnames)
        reads = sorted({(w >> 8) - CGB_VAR_V1 for w in prog.code
                        if w & 0xff == TERM_OPCODES['TERM_VAR'] and CGB_VAR_V1 <= (w >> 8) < CGB_VAR_V2})
        return prog, tuple(reads)

    compiled_values = [one(text, int(kind), place, 'computed value %s' % name) for place, (name, text, kind) in enumerate(values)]
    compiled_terms = [one(text, int(kind), len(values), 'energy term %d' % k) for k, (text, kind) in enumerate(terms)]
    return CustomGBPrograms([p for p, _ in compiled_values], [p for p, _ in compiled_terms], types,
                            [r for _, r in compiled_values], [r for _, r in compiled_terms], list(gnames))


def compile_polynomial(coefficients, scale, shift, operand):
    """Scalar program (amm_expr_eval_scalar) for sum_k coefficients[k] * u^k with u = scale * operand + shift: the first local holds u,
    one HORNER word per coefficient (top <- top * u + c)."""
    prog = Program()
    if isinstance(operand, Deferred):
        prog.emit('CONST', prog.const(operand.const))
        for k, coef in sorted(operand.terms.items()):
            prog.emit('DEVG', k)
            if coef != 1.0:
                prog.emit('CONST', prog.const(coef))
                prog.emit('MUL')
            prog.emit('ADD')
    else:
        prog.emit('CONST', prog.const(float(operand)))
    prog.emit('CONST', prog.const(scale))
    prog.emit('MUL')
    prog.emit('CONST', prog.const(shift))
    prog.emit('ADD')
    prog.emit('STORE', 0)
    prog.emit('CONST', prog.const(coefficients[-1]))
    for c in reversed(coefficients[:-1]):
        prog.consts.append(float(c))          # (no search for equal constants: their order is the polynomial's)
        prog.emit('HORNER', len(prog.consts) - 1)
    return prog


def compile_scalar(text, env, rng=None, predicate=None, keep=None):
    """Compile a GLOBAL expression (addComputeGlobal) whose operands include deferred values (Deferred: const + sum coef * scalar[k],
    the scalars living in a device buffer) into a postfix program for amm_expr_eval_scalar: numbers become constants, a Deferred its
    linear form over DEVG operands, `deriv(energy, p)` what env['__deriv__'] returns, `gaussian` / `uniform` one host draw each.
    `predicate` / `keep` (values as in env): the program's value is select(predicate, expression, keep) -- a step inside an
    if-block whose condition waits on the device."""
    main, defs = split_definitions(text)
    prog = Program()
    local_of, in_progress, draws = {}, set(), {}

    def value(v):
        if isinstance(v, Deferred):
            prog.emit('CONST', prog.const(v.const))
            for k, coef in sorted(v.terms.items()):
                prog.emit('DEVG', k)
                if coef != 1.0:
                    prog.emit('CONST', prog.const(coef))
                    prog.emit('MUL')
                prog.emit('ADD')
        else:
            prog.emit('CONST', prog.const(float(v)))

    def gen(node):
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            prog.emit('CONST', prog.const(node.value))
        elif isinstance(node, ast.Name):
            name = node.id
            if name in defs:
                if name not in local_of:
                    if name in in_progress:
                        raise ExpressionError('circular auxiliary definition: ' + name)
                    if len(local_of) + len(in_progress) >= MAX_LOCALS:
                        raise ExpressionError('too many auxiliary definitions')
                    in_progress.add(name)
                    gen(_parse(defs[name]))
                    in_progress.discard(name)
                    local_of[name] = len(local_of)
                    prog.emit('STORE', local_of[name])
                prog.emit('LOAD', local_of[name])
            elif name in ('gaussian', 'uniform', 'random'):
                key = 'gaussian' if name == 'gaussian' else 'uniform'
                if key not in draws:
                    if rng is None:
                        raise ExpressionError('random numbers in a global expression need a generator')
                    draws[key] = float(rng.standard_normal()) if key == 'gaussian' else float(rng.random())
                prog.emit('CONST', prog.const(draws[key]))
            elif name in env and not callable(env[name]):
                value(env[name])
            else:
                raise ExpressionError('unknown symbol in global expression: ' + name)
        elif isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            gen(node.operand)
            if isinstance(node.op, ast.USub):
                prog.emit('NEG')
        elif isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div, ast.Pow)):
            if isinstance(node.op, ast.Pow):
                e = node.right
                neg = isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.USub)
                ev = e.operand if neg else e
                if isinstance(ev, ast.Constant) and float(ev.value) == int(ev.value) and abs(int(ev.value)) < 1 << 20:
                    gen(node.left)
                    prog.emit('POWI', -int(ev.value) if neg else int(ev.value))
                    return
            gen(node.left)
            gen(node.right)
            prog.emit({ast.Add: 'ADD', ast.Sub: 'SUB', ast.Mult: 'MUL', ast.Div: 'DIV', ast.Pow: 'POW'}[type(node.op)])
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == 'deriv' and len(node.args) == 2 \
                and all(isinstance(a, ast.Name) for a in node.args):
            if '__deriv__' not in env:
                raise ExpressionError('deriv() is not available in this context')
            value(env['__deriv__'](node.args[0].id, node.args[1].id))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and not node.keywords:
            fn = node.func.id
            if fn not in OPCODES or fn.isupper() or len(node.args) != _ARITY.get(fn, 1):
                raise ExpressionError('unsupported function call: %s/%d' % (fn, len(node.args)))
            for a in node.args:
                gen(a)
            prog.emit(fn)
        else:
            raise ExpressionError('unsupported syntax in expression: ' + ast.dump(node))

    if predicate is not None:
        value(predicate)
    gen(_parse(main))
    if predicate is not None:
        value(keep)
        prog.emit('select')
    return prog


_HOST_FUNCS = dict(sqrt=math.sqrt, exp=math.exp, log=math.log, sin=math.sin, cos=math.cos, tan=math.tan, asin=math.asin,
                   acos=math.acos, atan=math.atan, sinh=math.sinh, cosh=math.cosh, tanh=math.tanh, erf=math.erf,
                   erfc=math.erfc, abs=abs, floor=math.floor, ceil=math.ceil, atan2=math.atan2, min=min, max=max,
                   step=lambda x: 1.0 if x >= 0 else 0.0, delta=lambda x: 1.0 if x == 0 else 0.0,
                   select=lambda c, a, b: a if c != 0 else b)


def eval_global(text, env, rng=None, functions=None):
    """Value of a global expression (addComputeGlobal) for the variable values in `env`; `rng` (numpy Generator)
    supplies `gaussian` / `uniform` (one draw of each per evaluation); functions: name -> callable of further functions the text may
    call (the tabulated functions of a pair text, for the symmetry check)."""
    main, defs = split_definitions(text)
    cache, draws, in_progress = {}, {}, set()

    def value_of(name):
        if name in defs:
            if name not in cache:
                if name in in_progress:
                    raise ExpressionError('circular auxiliary definition: ' + name)
                in_progress.add(name)
                cache[name] = ev(_parse(defs[name]))
                in_progress.discard(name)
            return cache[name]
        if name in ('gaussian', 'uniform', 'random'):
            key = 'gaussian' if name == 'gaussian' else 'uniform'
            if key not in draws:
                if rng is None:
                    raise ExpressionError('random numbers in a global expression need a generator')
                draws[key] = float(rng.standard_normal()) if key == 'gaussian' else float(rng.random())
            return draws[key]
        if name in env:
            return env[name] if isinstance(env[name], Deferred) else float(env[name])
        raise ExpressionError('unknown symbol in global expression: ' + name)

    def ev(node):
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return float(node.value)
        if isinstance(node, ast.Name):
            return value_of(node.id)
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = ev(node.operand)
            return -v if isinstance(node.op, ast.USub) else v
        if isinstance(node, ast.BinOp):
            a, b = ev(node.left), ev(node.right)
            if isinstance(node.op, ast.Add):
                return a + b
            if isinstance(node.op, ast.Sub):
                return a - b
            if isinstance(node.op, ast.Mult):
                return a * b
            if isinstance(node.op, ast.Div):
                return a / b
            if isinstance(node.op, ast.Pow):
                return a ** b
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == 'deriv' and len(node.args) == 2 \
                and all(isinstance(a, ast.Name) for a in node.args):
            # deriv(energy, parameter): supplied by the engine (force kernels), integrators.py:735
            if '__deriv__' not in env:
                raise ExpressionError('deriv() is not available in this context')
            value = env['__deriv__'](node.args[0].id, node.args[1].id)
            return value if isinstance(value, Deferred) else float(value)
        if functions and isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in functions and not node.keywords:
            return float(functions[node.func.id](*[ev(a) for a in node.args]))
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in _HOST_FUNCS and not node.keywords:
            if len(node.args) != _ARITY.get(node.func.id, 1):
                raise ExpressionError('unsupported function call: %s/%d' % (node.func.id, len(node.args)))
            return float(_HOST_FUNCS[node.func.id](*[ev(a) for a in node.args]))
        raise ExpressionError('unsupported syntax in expression: ' + ast.dump(node))

    return ev(_parse(main))


@functools.lru_cache(maxsize=4096)
def symbols(text):
    """Names referenced by an expression (auxiliary definitions expanded, their own names removed)."""
    main, defs = split_definitions(text)
    found = set()
    for part in [main] + list(defs.values()):
        for node in ast.walk(_parse(part)):
            if isinstance(node, ast.Name):
                found.add(node.id)
    return frozenset(found - set(defs) - set(_HOST_FUNCS))
