// atomsmm_amd/csrc/pair_expr_vm.h -- the pair-expression interpreter (device side) of k_pair_expr (pair_expr.hip): the energy text of
// a CustomNonbondedForce that is none of the hand-written families, compiled by atomsmm_amd/expr.py (compile_pair) into the postfix
// code of expr_vm.h, evaluated per pair together with its derivative in r.
//
// Forward mode: every stack slot and every local is a pair (value, d/dr).  X_PAIR_R pushes (r, 1); constants, globals and the
// per-particle parameters push (x, 0), so that a mixing rule -- a definition without r -- carries a zero derivative through every
// op on its own.  The chain rule goes through pexpr_chain: a factor whose operand has derivative exactly zero contributes an exact
// zero whatever f'(x) is (sqrt(eps1*eps2) at eps = 0 has f' = inf; the pair's energy does not depend on r through it).
// Discontinuous ops follow Lepton: step, delta, floor, ceil have derivative 0, abs takes the sign of its operand, min / max / select
// carry the derivative of the operand they return.
//
// Tabulated functions (addTabulatedFunction): X_TAB_C1 / X_TAB_D1 / X_TAB_D2 replace their arguments with the value of
// table `arg` of the force (pexpr_table).  A Continuous1DFunction carries its spline's derivative through pexpr_chain; the discrete
// ones have derivative 0.  The tables live in ONE device allocation -- AMM_PEXPR_MAXTABLES descriptors, then the doubles -- read from
// global memory (every lane reads the same few lines: L2), so the LDS of a block is what it was without them.
#pragma once
#include "expr_force.h"        // PairExprProg and its limits, the program holder
#include "expr_vm.h"

#define AMM_PEXPR_STACK 16
#define AMM_PEXPR_LOCALS 16
#define AMM_PEXPR_PARAMS 3          // per-particle doubles a neighbour row carries per atom (charge slot, two Lennard-Jones slots)
#define AMM_PEXPR_MAXTABLES 8       // tabulated functions of one force
#define AMM_PEXPR_STRIDE 256        // lanes per block of k_pair_expr / k_term_expr: slot k of lane t is s_stack[k * 256 + t]

// opcodes beside those of expr_vm.h (X_BUF, X_MASS, X_GAUSS, X_UNIFORM, X_DEVG, X_OUT and X_HORNER are not pair ops)
enum { X_PAIR_R = 50, X_PAIR_P1 = 51, X_PAIR_P2 = 52 };
// ... and the leaves of a term expression (term_expr_vm.h): the term's geometric variable k, its parameter k
enum { X_TERM_VAR = 53, X_TERM_P = 54 };
// ... and the tabulated functions of a pair expression: table `arg` at the top of the stack (X_TAB_D2: at the two topmost, x below y)
enum { X_TAB_C1 = 55, X_TAB_D1 = 56, X_TAB_D2 = 57 };

// One tabulated function as the device reads it.  kind: AMM_TABLE_* (atomsmm_hip.h).  Continuous: nx knots lo .. hi at spacing h, data =
// nx - 1 records (a, b, c, d) of the interval's cubic a + u (b + u (c + u d)), u = t - knot; discrete: data = nx (* ny) values,
// values[i + nx * j].  off: where the table's doubles begin behind the descriptors (a multiple of 4: records are 32-byte aligned).
struct PairTableDesc {
    int kind, nx, ny, off;
    double lo, hi, h, inv_h;
};

// host side of a generic pair force (PairForce::expr)
struct PairExpr {
    ExprProgram prog;
    bool uses_tables = false;                   // the program has X_TAB_* words: no launch before amm_pair_expr_set_tables
    int n_tables = 0;
    PairTableDesc tabs[AMM_PEXPR_MAXTABLES];    // as uploaded (a re-upload keeps kinds and sizes)
    size_t n_data = 0;                          // doubles behind the descriptors
    PairTableDesc *d_tabs = nullptr;            // descriptors [AMM_PEXPR_MAXTABLES], then the doubles: one allocation, freed with the force
};

// non-zero + message naming the limit that a program exceeds, or a word that is no pair op / leaves the stack or the locals
int amm_pair_expr_validate(const int32_t *code, int ncode, int nconst, int nglobal);

#ifdef __HIPCC__
__device__ __forceinline__ double pexpr_chain(double fprime, double xd) { return xd == 0.0 ? 0.0 : fprime * xd; }

__device__ __forceinline__ double pexpr_powi(double b, int n) {
#pragma clang fp contract(off)
    int e = n < 0 ? -n : n;
    double r = 1.0, q = b;
    while (e) {
        if (e & 1) r *= q;
        q *= q;
        e >>= 1;
    }
    return n < 0 ? 1.0 / r : r;
}

// The transcendental ops are CALLED, one copy per kernel (as expr_run is): inlined into the dispatch loop, the constants of their
// polynomials are hoisted out of it and stay live across every op (388 registers, one wavefront per SIMD).  (f(x), f'(x)):
static __device__ __noinline__ double2 pexpr_fn(int op, double x) {
#pragma clang fp contract(off)
    double v = 0.0, fp = 0.0;
    switch (op) {
    case X_EXP: v = exp(x); fp = v; break;
    case X_LOG: v = log(x); fp = 1.0 / x; break;
    case X_SIN: v = sin(x); fp = cos(x); break;
    case X_COS: v = cos(x); fp = -sin(x); break;
    case X_TAN: v = tan(x); fp = 1.0 + v * v; break;
    case X_ASIN: v = asin(x); fp = 1.0 / sqrt(1.0 - x * x); break;
    case X_ACOS: v = acos(x); fp = -1.0 / sqrt(1.0 - x * x); break;
    case X_ATAN: v = atan(x); fp = 1.0 / (1.0 + x * x); break;
    case X_SINH: v = sinh(x); fp = cosh(x); break;
    case X_COSH: v = cosh(x); fp = sinh(x); break;
    case X_TANH: v = tanh(x); fp = 1.0 - v * v; break;
    case X_ERF: v = erf(x); fp = 1.1283791670955125739 * exp(-(x * x)); break;
    case X_ERFC: v = erfc(x); fp = -(1.1283791670955125739 * exp(-(x * x))); break;
    default: break;
    }
    return make_double2(v, fp);
}
// (a^b, d/da, d/db) of the general power: b a^(b-1) and a^b log a
static __device__ __noinline__ double3 pexpr_pow(double a, double b, bool with_log) {
#pragma clang fp contract(off)
    const double v = pow(a, b);
    return make_double3(v, b * pow(a, b - 1.0), with_log ? v * log(a) : 0.0);
}
static __device__ __noinline__ double pexpr_atan2(double y, double x) { return atan2(y, x); }

// (f, f') of tabulated function `idx` at x (X_TAB_D2: at (x, y)).  CALLED, as the transcendental ops are: the descriptor, the address
// arithmetic and the NaN constant live in here, not across the dispatch loop.  Every index is clamped into its table BEFORE the load,
// whatever the argument is (NaN, inf, beyond int): no input reads outside the allocation.
//   continuous: 0 outside [lo, hi] (value and derivative); inside, the cubic of interval k = min(floor((x - lo) / h), nx - 2), so that
//               x == hi is the end of the last interval; a NaN argument gives NaN through u.
//   discrete:   values[rint(x)] (values[rint(x) + nx * rint(y)]); an index outside the table, or NaN, gives NaN.  Derivative 0.
static __device__ __noinline__ double2 pexpr_table(const PairTableDesc *tabs, int op, int idx, double x, double y) {
#pragma clang fp contract(off)
    const PairTableDesc *T = tabs + idx;
    const double *data = reinterpret_cast<const double *>(tabs + AMM_PEXPR_MAXTABLES) + T->off;
    const int nx = T->nx;
    if (op == X_TAB_C1) {
        const double lo = T->lo;
        if (x < lo || x > T->hi) return make_double2(0.0, 0.0);
        const double s = (x - lo) * T->inv_h;
        int k = (s >= 0.0 && s < (double)nx) ? (int)s : 0;         // (NaN: 0)
        k = min(max(k, 0), nx - 2);
        const double u = (x - lo) - (double)k * T->h;
        const double2 ab = *reinterpret_cast<const double2 *>(data + 4 * (size_t)k);
        const double2 cd = *reinterpret_cast<const double2 *>(data + 4 * (size_t)k + 2);
        return make_double2(ab.x + u * (ab.y + u * (cd.x + u * cd.y)), ab.y + u * (2.0 * cd.x + u * (3.0 * cd.y)));
    }
    const double rx = rint(x), ry = op == X_TAB_D2 ? rint(y) : 0.0;
    const int ny = op == X_TAB_D2 ? T->ny : 1;
    const bool inside = rx >= 0.0 && rx < (double)nx && ry >= 0.0 && ry < (double)ny;          // (false for NaN)
    const int i = min(max(inside ? (int)rx : 0, 0), nx - 1), j = min(max(inside ? (int)ry : 0, 0), ny - 1);
    const double v = data[(size_t)i + (size_t)nx * j];
    return make_double2(inside ? v : __builtin_nan(""), 0.0);
}

// The leaves of a pair expression: r with derivative 1, pa / pb the parameters of the row atom (<name>1) and of the neighbour (<name>2).
// TAB: the program has X_TAB_* words, and `tabs` the force's tables; without them the words compile to nothing and the interpreter is
// the one it was before there were any.
template <bool TAB>
struct PairLeaves {
    static constexpr bool kPair = true;
    static constexpr bool kTables = TAB;
    static constexpr int kStride = AMM_PEXPR_STRIDE;
    double r;
    const double *pa, *pb;
    const PairTableDesc *tabs;
};

// Does a leaves type run the table words?  Only one that says so with a member kTables (and then has `tabs`): PairLeaves<true>, and
// the CgbLeaves of custom_gb.hip, whose other leaves are the term words.  TermLeaves and CvLeaves declare nothing and compile the
// words to nothing, as before.
template <class L, class = void>
struct pexpr_has_tables {
    static constexpr bool value = false;
};
template <class L>
struct pexpr_has_tables<L, decltype((void)L::kTables)> {
    static constexpr bool value = L::kTables;
};

// E and its derivative along the leaves' seed.  code / consts / globals: the block's LDS copies.  The program is the same for every
// lane, so the word is made scalar (readfirstlane) and the dispatch is a scalar branch.  The top of the stack lives in registers
// (tv, td): a unary op touches no memory, a binary op reads one slot.  The elements below it are the lane's column of an LDS strip --
// st[k * AMM_PEXPR_STRIDE], one (value, derivative) record of 16 bytes per slot, neighbouring lanes in neighbouring records
// (conflict-free) -- and the locals are a private array.  `Leaves`: PairLeaves, or the TermLeaves of term_expr_vm.h -- the words of
// the other kind compile to nothing -- or the CvLeaves of cv.hip, whose strip is 32 lanes wide (Leaves::kStride: lanes of the strip), or
// the CgbLeaves of custom_gb.hip (term words and table words).
template <class Leaves>
__device__ __forceinline__ void pexpr_run(const int *code, int ncode, const double *consts, const double *globals, const Leaves &leaves,
                                          double2 *st, double &E, double &dE) {
#pragma clang fp contract(off)
    double lv[AMM_PEXPR_LOCALS], ld[AMM_PEXPR_LOCALS];
    double tv = 0.0, td = 0.0;
    int sp = 0;                     // elements on the stack: 0 .. sp - 2 in the strip, sp - 1 in (tv, td)
#define PEXPR_PUSH(V, D)                                                  \
    do {                                                                  \
        const double v_ = (V), d_ = (D);                                  \
        if (sp) st[(sp - 1) * Leaves::kStride] = make_double2(tv, td);   \
        tv = v_;                                                          \
        td = d_;                                                          \
        ++sp;                                                             \
    } while (0)
#define PEXPR_UNARY(VALUE, FPRIME)                 \
    do {                                           \
        const double x = tv;                       \
        const double v = (VALUE);                  \
        (void)x;                                   \
        td = pexpr_chain((FPRIME), td);            \
        tv = v;                                    \
    } while (0)
    for (int pc = 0; pc < ncode; ++pc) {
        const int word = __builtin_amdgcn_readfirstlane(code[pc]), op = word & 0xff, arg = word >> 8;
        switch (op) {
        case X_CONST: PEXPR_PUSH(consts[arg], 0.0); break;
        case X_GLOBAL: PEXPR_PUSH(globals[arg], 0.0); break;
        case X_PAIR_R: if constexpr (Leaves::kPair) PEXPR_PUSH(leaves.r, 1.0); break;
        case X_PAIR_P1: if constexpr (Leaves::kPair) PEXPR_PUSH(arg == 0 ? leaves.pa[0] : (arg == 1 ? leaves.pa[1] : leaves.pa[2]), 0.0); break;
        case X_PAIR_P2: if constexpr (Leaves::kPair) PEXPR_PUSH(arg == 0 ? leaves.pb[0] : (arg == 1 ? leaves.pb[1] : leaves.pb[2]), 0.0); break;
        case X_TERM_VAR: if constexpr (!Leaves::kPair) PEXPR_PUSH(leaves.var(arg), leaves.seed(arg)); break;
        case X_TERM_P: if constexpr (!Leaves::kPair) PEXPR_PUSH(leaves.param(arg), 0.0); break;
        // The table words are cases of the instantiation for programs that HAVE them only (PairLeaves<true>): the compiler lowers this
        // switch to a tree of scalar compares and lays the cases out as it sees fit, and three more cases cost every other word of a
        // program without tables 1.6 % (as cases) to 8 % (behind a range test in the default) on the MI355X -- DESIGN.md 3.PT.
        case X_TAB_C1: case X_TAB_D1:
            if constexpr (pexpr_has_tables<Leaves>::value) {
                const double2 f = pexpr_table(leaves.tabs, op, arg, tv, 0.0);
                tv = f.x;
                td = op == X_TAB_C1 ? pexpr_chain(f.y, td) : 0.0;
            }
            break;
        case X_TAB_D2:
            if constexpr (pexpr_has_tables<Leaves>::value) {
                const double2 lhs = st[(sp - 2) * Leaves::kStride];
                --sp;
                tv = pexpr_table(leaves.tabs, op, arg, lhs.x, tv).x;
                td = 0.0;
            }
            break;
        case X_LOAD: PEXPR_PUSH(lv[arg], ld[arg]); break;
        case X_STORE: {
            lv[arg] = tv;
            ld[arg] = td;
            --sp;
            if (sp) {
                const double2 t = st[(sp - 1) * Leaves::kStride];
                tv = t.x;
                td = t.y;
            }
        } break;
        case X_ADD: case X_SUB: case X_MUL: case X_DIV: case X_POW: case X_MIN: case X_MAX: case X_ATAN2: {
            const double2 lhs = st[(sp - 2) * Leaves::kStride];
            const double a = lhs.x, ad = lhs.y, b = tv, bd = td;
            --sp;
            if (op == X_ADD) {
                tv = a + b;
                td = ad + bd;
            } else if (op == X_SUB) {
                tv = a - b;
                td = ad - bd;
            } else if (op == X_MUL) {
                tv = a * b;
                td = pexpr_chain(b, ad) + pexpr_chain(a, bd);
            } else if (op == X_DIV) {
                const double q = a / b;
                tv = q;
                td = (ad == 0.0 && bd == 0.0) ? 0.0 : (ad - pexpr_chain(q, bd)) / b;
            } else if (op == X_POW) {
                // b' = 0: b a^(b-1) a'; else the full form, the term in log a taken only then (a <= 0: the value is what pow gives)
                const double3 p = pexpr_pow(a, b, bd != 0.0);
                double d = pexpr_chain(p.y, ad);
                if (bd != 0.0) d = d + p.z * bd;
                tv = p.x;
                td = d;
            } else if (op == X_MIN) {
                td = a <= b ? ad : bd;
                tv = fmin(a, b);
            } else if (op == X_MAX) {
                td = a >= b ? ad : bd;
                tv = fmax(a, b);
            } else {        // atan2(a, b)
                tv = pexpr_atan2(a, b);
                td = (ad == 0.0 && bd == 0.0) ? 0.0 : (b * ad - a * bd) / (b * b + a * a);
            }
        } break;
        case X_SELECT: {
            const double2 c = st[(sp - 3) * Leaves::kStride], a = st[(sp - 2) * Leaves::kStride];
            sp -= 2;
            const bool first = c.x != 0.0;
            tv = first ? a.x : tv;
            td = first ? a.y : td;
        } break;
        case X_NEG: tv = -tv; td = -td; break;
        case X_POWI: {
            const double x = tv;
            tv = pexpr_powi(x, arg);
            td = arg == 0 ? 0.0 : pexpr_chain((double)arg * pexpr_powi(x, arg - 1), td);
        } break;
        case X_SQRT: PEXPR_UNARY(sqrt(x), 0.5 / v); break;
        case X_EXP: case X_LOG: case X_SIN: case X_COS: case X_TAN: case X_ASIN: case X_ACOS: case X_ATAN: case X_SINH: case X_COSH:
        case X_TANH: case X_ERF: case X_ERFC: {
            const double2 f = pexpr_fn(op, tv);
            tv = f.x;
            td = pexpr_chain(f.y, td);
        } break;
        case X_ABS: td = tv >= 0.0 ? td : -td; tv = fabs(tv); break;
        case X_FLOOR: tv = floor(tv); td = 0.0; break;
        case X_CEIL: tv = ceil(tv); td = 0.0; break;
        case X_STEP: tv = tv >= 0.0 ? 1.0 : 0.0; td = 0.0; break;
        case X_DELTA: tv = tv == 0.0 ? 1.0 : 0.0; td = 0.0; break;
        default: break;
        }
    }
#undef PEXPR_PUSH
#undef PEXPR_UNARY
    E = tv;
    dE = td;
}

// E(r) and dE/dr of one pair
template <bool TAB>
__device__ __forceinline__ void pair_expr_run(const int *code, int ncode, const double *consts, const double *globals, double r,
                                              const double *pa, const double *pb, const PairTableDesc *tabs, double2 *st, double &E,
                                              double &dE) {
    pexpr_run(code, ncode, consts, globals, PairLeaves<TAB>{r, pa, pb, tabs}, st, E, dE);
}
#endif
