// atomsmm_amd/csrc/pair_expr.hip -- generic pair force: a CustomNonbondedForce whose energy text is none of the hand-written families
// (AMM_PAIR_EXPR), evaluated by interpreting the compiled text per pair (pair_expr_vm.h).
//
// Takes over what OpenMM does for any CustomNonbondedForce(energy) with CutoffPeriodic: per pair within the cutoff and not excluded,
// the energy expression and its derivative in r (Lepton differentiates the text; here the interpreter carries d/dr along).
//
// k_pair_expr walks the per-atom neighbour rows of pair.hip exactly as k_pair_nlist does -- same PairArgs, lanes per atom, front / back
// row entries, minimum image, r2 < rc2, fixed butterfly reduction, owner-computes without atomics, per-block energy partials with the
// factor 1/2 -- one row entry per lane and trip.  The row atom's three per-particle doubles are <name>1, the neighbour's <name>2; they
// are the RAW values of the force's per-particle parameters.  Every pair is evaluated from both rows, so the text must be symmetric
// under 1 <-> 2 (the host checks it: engine.py).
//
// Layout: code, constants and globals are staged once per block in LDS (2.8 KiB) and read back wave-uniformly.  The top of each
// lane's stack is a register pair; the 15 slots below it are the lane's column of an LDS strip (15 x 256 lanes x 16 B = 60 KiB per
// block: two blocks per CU, two wavefronts per SIMD -- the transcendental ops of the interpreter need more than 128 VGPRs anyway); the
// 16 locals are a private array.  DESIGN.md 3.PE has the resource figures and the measured cost.
#include <cstring>

#include "amm_ctx.h"
#include "device_utils.h"
#include "pair_args.h"
#include "pair_math.h"
#include "pair_expr_vm.h"
#include "term_expr_vm.h"

// EN: with the energy.  TAB: the program has tabulated-function words (a kernel of its own, so that a program without them runs the
// code it ran before there were any).
template <bool EN, bool TAB>
__global__ void __launch_bounds__(256) k_pair_expr(PairArgs A, const PairExprProg *__restrict__ prog, const PairTableDesc *__restrict__ tabs,
                                                   double rc2, double rswitch, double inv_sw_dr, int use_switch, double sign) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_PEXPR_STRIDE];      // all but the top of every lane's stack
    const int ncode = prog->ncode;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    __syncthreads();
    const int lpa = 1 << A.lpa_shift;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = tid >> A.lpa_shift;
    const int sub = tid & (lpa - 1);
    const int s = A.s_begin + a;
    const bool valid = s < A.s_end;
    double fx = 0.0, fy = 0.0, fz = 0.0, esum = 0.0;
    if (valid) {
        const double4 pi = A.posq_s[s];
        const double2 li = A.lj_s[s];
        const double pa[AMM_PEXPR_PARAMS] = {pi.w, li.x, li.y};
        const int nfront = A.nnb[a];
        const int nn = A.nnb_total ? A.nnb_total[a] : nfront;
        const int *row = A.nl + (size_t)a * A.cap;
        const int back = A.cap - 1 + nfront;
        for (int k = sub; k < nn; k += lpa) {
            const int j = row[k < nfront ? k : back - k];
            const double4 pj = A.posq_s[j];
            const double2 lj = A.lj_s[j];
            const double dx = amm_min_image(pi.x - pj.x, A.box.L[0], A.box.invL[0]);
            const double dy = amm_min_image(pi.y - pj.y, A.box.L[1], A.box.invL[1]);
            const double dz = amm_min_image(pi.z - pj.z, A.box.L[2], A.box.invL[2]);
            const double r2 = dx * dx + dy * dy + dz * dz;
            if (r2 < rc2) {
                const double r = sqrt(r2);
                const double pb[AMM_PEXPR_PARAMS] = {pj.w, lj.x, lj.y};
                double e, de;
                pair_expr_run<TAB>(s_code, ncode, s_consts, s_globals, r, pa, pb, tabs, s_stack + threadIdx.x, e, de);
                if (use_switch && r > rswitch) {
                    // OpenMM's built-in switch, S = 1 - 10 t^3 + 15 t^4 - 6 t^5, applied after the program
                    const double t = (r - rswitch) * inv_sw_dr;
                    const double S = 1.0 + (t * t * t) * (-10.0 + t * (15.0 - 6.0 * t));
                    const double omt = 1.0 - t;
                    const double dS = (-30.0 * (t * t) * (omt * omt)) * inv_sw_dr;
                    de = S * de + dS * e;
                    e = S * e;
                }
                const double fr = -(sign * de) / r;
                fx += fr * dx;
                fy += fr * dy;
                fz += fr * dz;
                if (EN) esum += sign * e;
            }
        }
    }
    // combine the lpa partial sums of each atom (fixed butterfly order -> deterministic)
    for (int off = lpa >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
    }
    if (valid && sub == 0) {
        const int i = A.sorted_out ? s - A.s_begin : A.perm[s];
        if (A.accumulate) {
            A.force[3 * i] += fx;
            A.force[3 * i + 1] += fy;
            A.force[3 * i + 2] += fz;
        } else {
            A.force[3 * i] = fx;
            A.force[3 * i + 1] = fy;
            A.force[3 * i + 2] = fz;
        }
    }
    if (EN) block_energy_store_256(esum, A.epart, 0.5);
}

// the launch of amm_pair_eval_impl for a force of family AMM_PAIR_EXPR (grid: one lane group per row of the slice, as k_pair_nlist)
int amm_pair_expr_launch(amm_ctx *ctx, PairForce *pf, const PairArgs &A, dim3 grid, bool en) {
    if (!pf->expr || !pf->expr->prog.d) {
        amm_set_error("pair-expression force (AMM_PAIR_EXPR) without a program");
        return 1;
    }
    if (A.active || A.gsame) {
        amm_set_error("pair-expression force (AMM_PAIR_EXPR): filtered rows and dual evaluation are not for this family");
        return 1;
    }
    if (pf->expr->uses_tables && !pf->expr->d_tabs) {
        amm_set_error("pair-expression force (AMM_PAIR_EXPR): the program reads tabulated functions and none are set: amm_pair_expr_set_tables");
        return 1;
    }
    const PairConsts &c = pf->pc;
    const PairTableDesc *tabs = pf->expr->uses_tables ? pf->expr->d_tabs : nullptr;
    const int use_switch = (c.flags & AMM_SWITCH) ? 1 : 0;
    const double inv_sw_dr = use_switch ? 1.0 / (c.rc - c.rswitch) : 0.0;
#define AMM_PEXPR_LAUNCH(EN, TAB) \
    hipLaunchKernelGGL((k_pair_expr<EN, TAB>), grid, dim3(256), 0, ctx->stream, A, pf->expr->prog.d, tabs, c.rc2, c.rswitch, inv_sw_dr, use_switch, c.sign)
    if (tabs) {
        if (en) AMM_PEXPR_LAUNCH(true, true);
        else AMM_PEXPR_LAUNCH(false, true);
    } else {
        if (en) AMM_PEXPR_LAUNCH(true, false);
        else AMM_PEXPR_LAUNCH(false, false);
    }
#undef AMM_PEXPR_LAUNCH
    return 0;
}

// ---- host: program checks ----
int amm_pair_expr_validate(const int32_t *code, int ncode, int nconst, int nglobal) {
    return amm_expr_program_validate("amm_pair_expr_create", code, ncode, nconst, nglobal, -1, 0);
}

int amm_expr_program_validate(const char *who, const int32_t *code, int ncode, int nconst, int nglobal, int term_vars, int term_params,
                              bool term_tables) {
    auto fail = [who](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what);
        return 1;
    };
    const bool pair = term_vars < 0;
    if (ncode < 1 || ncode > AMM_PEXPR_MAXCODE) return fail("the program has " + std::to_string(ncode) + " code words (limit " + std::to_string(AMM_PEXPR_MAXCODE) + ")");
    if (nconst < 0 || nconst > AMM_PEXPR_MAXCONST) return fail("the program has " + std::to_string(nconst) + " constants (limit " + std::to_string(AMM_PEXPR_MAXCONST) + ")");
    if (nglobal < 0 || nglobal > AMM_PEXPR_MAXGLOBAL) return fail("the program has " + std::to_string(nglobal) + " globals (limit " + std::to_string(AMM_PEXPR_MAXGLOBAL) + ")");
    int sp = 0;
    for (int pc = 0; pc < ncode; ++pc) {
        const int op = code[pc] & 0xff, arg = code[pc] >> 8;
        int pops = 1, pushes = 1;          // (the unary functions)
        switch (op) {
        case X_CONST: pops = 0; if (arg < 0 || arg >= nconst) return fail("constant index out of range"); break;
        case X_GLOBAL: pops = 0; if (arg < 0 || arg >= nglobal) return fail("global index out of range"); break;
        case X_PAIR_R: pops = 0; if (!pair) return fail("opcode " + std::to_string(op) + " is not a term-expression op"); break;
        case X_TERM_VAR: pops = 0; if (pair) return fail("opcode " + std::to_string(op) + " is not a pair-expression op"); if (arg < 0 || arg >= term_vars) return fail("variable index out of range (the kind has " + std::to_string(term_vars) + ")"); break;
        case X_TERM_P: pops = 0; if (pair) return fail("opcode " + std::to_string(op) + " is not a pair-expression op"); if (arg < 0 || arg >= term_params) return fail("per-term parameter index out of range (the force has " + std::to_string(term_params) + ")"); break;
        case X_PAIR_P1: case X_PAIR_P2: pops = 0; if (!pair) return fail("opcode " + std::to_string(op) + " is not a term-expression op"); if (arg < 0 || arg >= AMM_PEXPR_PARAMS) return fail("per-particle parameter index out of range (limit " + std::to_string(AMM_PEXPR_PARAMS) + ")"); break;
        case X_TAB_C1: case X_TAB_D1: case X_TAB_D2: pops = op == X_TAB_D2 ? 2 : 1; if (!pair && !term_tables) return fail("opcode " + std::to_string(op) + " is not a term-expression op"); if (arg < 0 || arg >= AMM_PEXPR_MAXTABLES) return fail("tabulated-function index out of range (limit " + std::to_string(AMM_PEXPR_MAXTABLES) + ")"); break;
        case X_LOAD: pops = 0; if (arg < 0 || arg >= AMM_PEXPR_LOCALS) return fail("local index out of range (limit " + std::to_string(AMM_PEXPR_LOCALS) + ")"); break;
        case X_STORE: pushes = 0; if (arg < 0 || arg >= AMM_PEXPR_LOCALS) return fail("local index out of range (limit " + std::to_string(AMM_PEXPR_LOCALS) + ")"); break;
        case X_ADD: case X_SUB: case X_MUL: case X_DIV: case X_POW: case X_MIN: case X_MAX: case X_ATAN2: pops = 2; break;
        case X_SELECT: pops = 3; break;
        case X_NEG: case X_POWI: case X_SQRT: case X_EXP: case X_LOG: case X_SIN: case X_COS: case X_TAN: case X_ASIN: case X_ACOS: case X_ATAN:
        case X_SINH: case X_COSH: case X_TANH: case X_ERF: case X_ERFC: case X_ABS: case X_FLOOR: case X_CEIL: case X_STEP: case X_DELTA: break;
        default: return fail("opcode " + std::to_string(op) + (pair ? " is not a pair-expression op" : " is not a term-expression op"));
        }
        if (sp < pops) return fail("stack underflow at word " + std::to_string(pc));
        sp += pushes - pops;
        if (sp > AMM_PEXPR_STACK) return fail("stack depth exceeds " + std::to_string(AMM_PEXPR_STACK));
    }
    if (sp != 1) return fail("the program leaves " + std::to_string(sp) + " values on the stack (one expected)");
    return 0;
}

// ---- host: tabulated functions ----
static const char *table_word_name(int op) { return op == X_TAB_C1 ? "TAB_C1 (55)" : (op == X_TAB_D1 ? "TAB_D1 (56)" : "TAB_D2 (57)"); }
static const char *table_kind_name(int kind) {
    return kind == AMM_TABLE_CONTINUOUS1D ? "Continuous1DFunction" : (kind == AMM_TABLE_DISCRETE1D ? "Discrete1DFunction" : "Discrete2DFunction");
}
// doubles of a table of this kind and size
static size_t table_doubles(int kind, int nx, int ny) {
    return kind == AMM_TABLE_CONTINUOUS1D ? 4 * (size_t)(nx - 1) : (size_t)nx * (size_t)(kind == AMM_TABLE_DISCRETE2D ? ny : 1);
}

void amm_pair_expr_scan_tables(PairExpr *px) {
    px->uses_tables = false;
    for (int pc = 0; pc < px->prog.h.ncode; ++pc) {
        const int op = px->prog.h.code[pc] & 0xff;
        if (op == X_TAB_C1 || op == X_TAB_D1 || op == X_TAB_D2) px->uses_tables = true;
    }
}

int amm_pair_expr_tables(amm_ctx *ctx, PairExpr *px, int n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                         const int32_t *offsets, const double *data, int n_data) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_pair_expr_set_tables: " + what);
        return 1;
    };
    if (n_tables < 0 || n_tables > AMM_PEXPR_MAXTABLES) return fail(std::to_string(n_tables) + " tabulated functions (limit " + std::to_string(AMM_PEXPR_MAXTABLES) + ")");
    if (n_data < 0 || (n_tables > 0 && (!kinds || !dims || !ranges || !offsets || !data))) return fail("null argument");
    // the tables as the device will hold them: every table's doubles start at a multiple of 4
    PairTableDesc tabs[AMM_PEXPR_MAXTABLES];
    std::memset(tabs, 0, sizeof(tabs));
    size_t total = 0;
    for (int k = 0; k < n_tables; ++k) {
        PairTableDesc &T = tabs[k];
        const std::string which = "table " + std::to_string(k);
        T.kind = kinds[k];
        if (T.kind != AMM_TABLE_CONTINUOUS1D && T.kind != AMM_TABLE_DISCRETE1D && T.kind != AMM_TABLE_DISCRETE2D) return fail(which + ": unknown kind " + std::to_string(T.kind));
        T.nx = dims[2 * k];
        T.ny = T.kind == AMM_TABLE_DISCRETE2D ? dims[2 * k + 1] : 1;
        if (T.nx < (T.kind == AMM_TABLE_CONTINUOUS1D ? 2 : 1) || T.ny < 1 || T.nx > (1 << 24) || T.ny > (1 << 24) || (size_t)T.nx * (size_t)T.ny > ((size_t)1 << 26))
            return fail(which + " (" + table_kind_name(T.kind) + "): size " + std::to_string(T.nx) + " x " + std::to_string(T.ny) + " (a continuous function needs 2 knots, any table at most 2^26 values)");
        if (T.kind == AMM_TABLE_CONTINUOUS1D) {
            T.lo = ranges[2 * k];
            T.hi = ranges[2 * k + 1];
            if (!(T.lo < T.hi) || !std::isfinite(T.lo) || !std::isfinite(T.hi)) return fail(which + " (Continuous1DFunction): needs finite min < max");
            T.h = (T.hi - T.lo) / (double)(T.nx - 1);
            T.inv_h = (double)(T.nx - 1) / (T.hi - T.lo);
        }
        const size_t need = table_doubles(T.kind, T.nx, T.ny);
        if (offsets[k] < 0 || (size_t)offsets[k] + need > (size_t)n_data)
            return fail(which + " (" + table_kind_name(T.kind) + "): " + std::to_string(need) + " doubles at offset " + std::to_string(offsets[k]) + " do not lie in the " + std::to_string(n_data) + " given");
        T.off = (int)total;
        total += (need + 3) & ~(size_t)3;
    }
    // every table word of the program finds a table of its kind (the kind says how many arguments the word takes)
    for (int pc = 0; pc < px->prog.h.ncode; ++pc) {
        const int op = px->prog.h.code[pc] & 0xff, arg = px->prog.h.code[pc] >> 8;
        if (op != X_TAB_C1 && op != X_TAB_D1 && op != X_TAB_D2) continue;
        if (arg < 0 || arg >= n_tables) return fail(std::string("word ") + table_word_name(op) + " reads table " + std::to_string(arg) + ": " + std::to_string(n_tables) + " given");
        const int want = op == X_TAB_C1 ? AMM_TABLE_CONTINUOUS1D : (op == X_TAB_D1 ? AMM_TABLE_DISCRETE1D : AMM_TABLE_DISCRETE2D);
        if (tabs[arg].kind != want)
            return fail(std::string("word ") + table_word_name(op) + " takes a " + table_kind_name(want) + " (" + (op == X_TAB_D2 ? "2 arguments" : "1 argument") + "), table " + std::to_string(arg) + " is a " + table_kind_name(tabs[arg].kind));
    }
    if (px->d_tabs) {
        // a re-upload (updateParametersInContext): new values in tables of the same kinds and sizes
        if (n_tables != px->n_tables) return fail("the force has " + std::to_string(px->n_tables) + " tabulated functions, " + std::to_string(n_tables) + " given: their number cannot change");
        for (int k = 0; k < n_tables; ++k)
            if (tabs[k].kind != px->tabs[k].kind || tabs[k].nx != px->tabs[k].nx || tabs[k].ny != px->tabs[k].ny)
                return fail("table " + std::to_string(k) + " changed its kind or size (" + std::to_string(px->tabs[k].nx) + " x " + std::to_string(px->tabs[k].ny) + " -> " + std::to_string(tabs[k].nx) + " x " + std::to_string(tabs[k].ny) + "): a re-upload carries new values only");
    }
    const size_t bytes = sizeof(tabs) + total * sizeof(double);
    std::vector<char> host(bytes, 0);
    std::memcpy(host.data(), tabs, sizeof(tabs));
    double *out = reinterpret_cast<double *>(host.data() + sizeof(tabs));
    for (int k = 0; k < n_tables; ++k) std::copy(data + offsets[k], data + offsets[k] + table_doubles(tabs[k].kind, tabs[k].nx, tabs[k].ny), out + tabs[k].off);
    // ordered after any kernel already queued on the stream that reads the old tables
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (!px->d_tabs) AMM_HIP(hipMalloc(&px->d_tabs, bytes));
    AMM_HIP(hipMemcpy(px->d_tabs, host.data(), bytes, hipMemcpyHostToDevice));
    px->n_tables = n_tables;
    px->n_data = total;
    std::memcpy(px->tabs, tabs, sizeof(tabs));
    return 0;
}

void amm_pair_expr_free(PairExpr *px) {
    if (!px) return;
    px->prog.release();
    if (px->d_tabs) (void)hipFree(px->d_tabs);
    delete px;
}
