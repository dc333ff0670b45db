"""TEST INFRASTRUCTURE (checker only): the words of a scalar program (atomsmm_amd/expr.py: compile_scalar, compile_polynomial ->
amm_expr_eval_scalar) run by a few lines of Python, shared by tests/test_scalar_programs.py and tests/test_expr_semantics_host.py."""
import math

from atomsmm_amd import expr as X

OP = {v: k for k, v in X.OPCODES.items()}
FUN = dict(sqrt=math.sqrt, exp=math.exp, log=math.log, sin=math.sin, cos=math.cos, tan=math.tan, abs=abs, floor=math.floor, ceil=math.ceil,
           step=lambda x: 1.0 if x >= 0 else 0.0, delta=lambda x: 1.0 if x == 0 else 0.0, tanh=math.tanh, sinh=math.sinh, cosh=math.cosh,
           erf=math.erf, erfc=math.erfc, asin=math.asin, acos=math.acos, atan=math.atan)


def run(code, consts, scalars):
    """What csrc/expr.hip: k_expr_scalar does, word by word."""
    st, loc = [], {}
    for word in code:
        op, arg = OP[word & 0xff], word >> 8
        if op == 'CONST':
            st.append(consts[arg])
        elif op == 'DEVG':
            st.append(scalars[arg])
        elif op == 'OUT':
            scalars[arg] = st.pop()
        elif op == 'LOAD':
            st.append(loc[arg])
        elif op == 'STORE':
            loc[arg] = st.pop()
        elif op == 'HORNER':
            st.append(st.pop() * loc[0] + consts[arg])
        elif op in ('ADD', 'SUB', 'MUL', 'DIV', 'POW', 'min', 'max', 'atan2'):
            b, a = st.pop(), st.pop()
            st.append({'ADD': a + b, 'SUB': a - b, 'MUL': a * b, 'DIV': a / b if b else float('nan'), 'POW': a ** b if op == 'POW' else 0.0,
                       'min': min(a, b), 'max': max(a, b), 'atan2': math.atan2(a, b)}[op])
        elif op == 'NEG':
            st.append(-st.pop())
        elif op == 'POWI':
            st.append(st.pop() ** arg)
        elif op == 'select':
            no, yes, cond = st.pop(), st.pop(), st.pop()
            st.append(yes if cond != 0.0 else no)
        else:
            st.append(FUN[op](st.pop()))
    assert not st


def evaluate(prog, scalars, dst=99):
    scalars = dict(scalars)
    run(prog.code + [X.OPCODES['OUT'] | (dst << 8)], prog.consts, scalars)
    return scalars[dst]
