// atomsmm_amd/csrc/hbond.hip -- CustomHbondForce with ANY energy text (AMM_FORCE_HBOND): D donors (d1, d2, d3) against A acceptors
// (a1, a2, a3), every pair that is not excluded and whose distance(d1, a1) lies inside the cutoff contributes the text -- up to 16
// geometric variables distance / angle / dihedral over the six particles, per-donor, per-acceptor and global parameters -- compiled by
// atomsmm_amd/expr.py (compile_hbond) into the program of pair_expr_vm.h plus the variable table of expr_force.h (slots 0 .. 2 the
// donor's particles, 3 .. 5 the acceptor's).
//
// A compound-bond force is a short explicit list; this one is D x A pairs of which the cutoff (or the text) keeps a few per cent.  So
// it is an all-pairs kernel in the decomposition of gb.hip: TWO passes over ordered pairs -- donor rows against acceptor columns, then
// acceptor rows against donor columns -- each leaving forces on the particles of its own rows only, the energy summed in the donor
// pass.  One wavefront (a block of 64 lanes) owns a row, or one chunk of a row's columns; it scans 64 columns at a time (the cutoff
// on |d1 - a1|^2 with the minimum image when periodic, then the row's sorted exclusion list), and APPENDS the survivors with ballot +
// prefix count to a queue of column indices in LDS.  The interpreter runs only when 64 survivors wait, and once more at the end of
// the row: a draining lane computes its pair's V variables (compound_geom.h, the geometry of k_compound) into its own LDS row, runs
// pexpr_run once per variable with a one-hot seed and adds -dE/dv_k grad v_k of the row's own slots to nine register accumulators.
// A fixed-order butterfly sums the 64 lanes and lane 0 parks nine doubles per (row, chunk); k_hbond_gather, one lane per atom, adds
// the atom's (donor, role) and then (acceptor, role) records in record order, each over its chunks in chunk order.
//
// No atomics, fp contraction off, all fp64: the same positions give the same bits, and the energy and the force-only instantiation
// give the same forces.  No dynamically indexed private array of this file's own: the variable table and the values are read from
// LDS, the particles of a slot are picked by selects and every gradient has static indices.  DESIGN.md 3.HB has the resource
// figures and the measured cost.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "compound_geom.h"
#include "device_utils.h"
#include "term_expr_vm.h"

#define AMM_HB_LANES 64
#define AMM_HB_MAX_ROWS 32768

struct HbondPass {                      // rows against columns: 0 donors against acceptors, 1 acceptors against donors
    int n_rows = 0, n_cols = 0, chunks = 1, chunk_len = 64;
    size_t park_base = 0;               // first (row, chunk) record of the pass in d_park
    int *d_ex_ptr = nullptr, *d_ex_col = nullptr;   // CSR of a row's excluded columns, sorted
};

struct HbondForce {
    int D = 0, A = 0, n_vars = 0, n_dp = 0, n_ap = 0, periodic = 0, cutoff = 0;
    double rc = 0.0;
    int compact = 1;
    ExprProgram prog;
    VarTable *d_tab = nullptr;
    int *d_donors = nullptr, *d_acceptors = nullptr;    // [D][3], [A][3]; -1: the slot is not there
    double *d_dpar = nullptr, *d_apar = nullptr;        // [n_dp][D], [n_ap][A]
    HbondPass pass[2];
    double *d_park = nullptr;           // [(row, chunk) records of pass 0, then of pass 1][3 roles][3]
    double *d_epart = nullptr;          // [D * chunks of pass 0]
    int *d_count = nullptr;             // [D * chunks of pass 0] survivors of the last evaluation
    int *d_ref_ptr = nullptr;           // [n + 1] CSR per atom of its records ...
    int *d_rec_src = nullptr;           // ... each (donor, or D + acceptor) * 3 + role: donors first, in index order
    long long launches = 0;
    bool evaluated = false;
};

// The leaves of a hydrogen-bond text: variable k is TERM_VAR k, read from the lane's own row of values in LDS (entry k of lane t at
// vars[k * 64]); the seed is the one-hot of this run; parameter k is the donor's k-th, behind them the acceptor's, read
// parameter-major from global memory when the program asks for it.
struct HbondLeaves {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_HB_LANES;
    const double *vars;
    int hot, n_dp;
    const double *pd, *pa;
    size_t sd, sa;
    __device__ __forceinline__ double var(int k) const { return vars[k * AMM_HB_LANES]; }
    __device__ __forceinline__ double seed(int k) const { return k == hot ? 1.0 : 0.0; }
    __device__ __forceinline__ double param(int k) const { return k < n_dp ? pd[(size_t)k * sd] : pa[(size_t)(k - n_dp) * sa]; }
};

struct HbondArgs {
    int pass, n_rows, n_cols, chunks, chunk_len, n_vars, periodic, cutoff, n_dp, D, A;
    const int *donors, *acceptors;
    const double *dpar, *apar;
    const int *ex_ptr, *ex_col;
    const double *pos;
    double rc2;
    double *park;               // the pass's first record
    double *epart;
    int *count;
    Box box;
};

__device__ __forceinline__ int hb_pick(int s, int i0, int i1, int i2, int i3, int i4, int i5) {
    return s == 0 ? i0 : (s == 1 ? i1 : (s == 2 ? i2 : (s == 3 ? i3 : (s == 4 ? i4 : i5))));
}

// EN: the donor pass of an evaluation with energy.  COMPACT = false drains after every batch of 64 columns that has a survivor (the
// measurement of DESIGN.md 3.HB; option hbond_compact).
template <bool EN, bool COMPACT>
__global__ void __launch_bounds__(AMM_HB_LANES) k_hbond(HbondArgs A, const PairExprProg *__restrict__ prog, const VarTable *__restrict__ tab) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ int s_kind[AMM_COMPOUND_MAX_VARS];
    __shared__ int4 s_slot[AMM_COMPOUND_MAX_VARS];
    __shared__ double s_val[AMM_COMPOUND_MAX_VARS * AMM_HB_LANES];                 // value k of lane t: s_val[k * 64 + t]
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_HB_LANES];              // all but the top of every lane's stack
    __shared__ int s_queue[2 * AMM_HB_LANES];                                       // surviving columns that wait for the interpreter
    const int lane = threadIdx.x;
    const int ncode = prog->ncode;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    var_table_stage(tab, s_kind, s_slot);
    __syncthreads();
    const int row = blockIdx.x / A.chunks, chunk = blockIdx.x - row * A.chunks;     // (the grid is n_rows * chunks)
    const int begin = min(chunk * A.chunk_len, A.n_cols), end = min(begin + A.chunk_len, A.n_cols);
    const int *rows3 = A.pass ? A.acceptors : A.donors, *cols3 = A.pass ? A.donors : A.acceptors;
    const int r0 = rows3[3 * row], r1 = max(rows3[3 * row + 1], 0), r2 = max(rows3[3 * row + 2], 0);     // (a slot at -1 is read by no variable)
    const double x0 = A.pos[3 * r0], y0 = A.pos[3 * r0 + 1], z0 = A.pos[3 * r0 + 2];
    const int ex_begin = A.ex_ptr[row], ex_end = A.ex_ptr[row + 1];
    const int base = 3 * A.pass;                // the row's own slots: base .. base + 2
    const PosPlain pos{A.pos};
    double f0[3] = {0.0, 0.0, 0.0}, f1[3] = {0.0, 0.0, 0.0}, f2[3] = {0.0, 0.0, 0.0};
    double e_sum = 0.0;
    int n_pass = 0, qn = 0;
    for (int j0 = begin;; j0 += AMM_HB_LANES) {
        const bool last = j0 >= end;            // (wave-uniform: one more turn behind the columns, to drain what is left)
        if (!last) {
            const int col = j0 + lane;
            bool keep = col < end;
            if (keep) {
                const int c0 = cols3[3 * col];
                // donor minus acceptor in both passes: the two passes test the same number
                double dx = x0 - A.pos[3 * c0], dy = y0 - A.pos[3 * c0 + 1], dz = z0 - A.pos[3 * c0 + 2];
                if (A.pass) {
                    dx = -dx;
                    dy = -dy;
                    dz = -dz;
                }
                if (A.periodic) {
                    dx = amm_min_image(dx, A.box.L[0], A.box.invL[0]);
                    dy = amm_min_image(dy, A.box.L[1], A.box.invL[1]);
                    dz = amm_min_image(dz, A.box.L[2], A.box.invL[2]);
                }
                if (A.cutoff) keep = dx * dx + dy * dy + dz * dz < A.rc2;
                if (keep && ex_end > ex_begin) keep = !sorted_contains(A.ex_col, ex_begin, ex_end, col);      // the row's excluded columns
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) s_queue[qn + __popcll(mask & ((1ull << lane) - 1ull))] = col;      // (qn < 64 here: at most 127 entries)
            qn += __popcll(mask);
            __syncthreads();
        }
        if (COMPACT ? (qn >= AMM_HB_LANES || (last && qn > 0)) : qn > 0) {
            const int take = min(qn, AMM_HB_LANES);
            const bool act = lane < take;
            if (act) {
                const int col = s_queue[lane];
                const int dn = A.pass ? col : row, ac = A.pass ? row : col;
                int i0, i1, i2, i3, i4, i5;
                if (A.pass) {
                    i0 = cols3[3 * col];
                    i1 = max(cols3[3 * col + 1], 0);
                    i2 = max(cols3[3 * col + 2], 0);
                    i3 = r0;
                    i4 = r1;
                    i5 = r2;
                } else {
                    i0 = r0;
                    i1 = r1;
                    i2 = r2;
                    i3 = cols3[3 * col];
                    i4 = max(cols3[3 * col + 1], 0);
                    i5 = max(cols3[3 * col + 2], 0);
                }
                HbondLeaves L;
                L.vars = s_val + lane;
                L.n_dp = A.n_dp;
                L.pd = A.dpar + dn;
                L.sd = (size_t)A.D;
                L.pa = A.apar + ac;
                L.sa = (size_t)A.A;
                // turns 0 .. V - 1 publish the values; turns V .. 2V - 1 take dE/dv_k (a text without variables: one run, for the energy)
                const int V = A.n_vars, turns = V + max(V, 1);
                for (int it = 0; it < turns; ++it) {
                    const bool publish = it < V;
                    const int k = publish ? it : it - V;
                    double v = 0.0, rr = 1.0;
                    double g0[3] = {0.0, 0.0, 0.0}, g1[3] = {0.0, 0.0, 0.0}, g2[3] = {0.0, 0.0, 0.0}, g3[3] = {0.0, 0.0, 0.0};
                    int kind = 0;
                    int4 sl = make_int4(0, 0, 0, 0);
                    if (k < V) {
                        kind = s_kind[k];
                        sl = s_slot[k];
                        compound_variable(pos, kind, hb_pick(sl.x, i0, i1, i2, i3, i4, i5), hb_pick(sl.y, i0, i1, i2, i3, i4, i5),
                                          hb_pick(sl.z, i0, i1, i2, i3, i4, i5), hb_pick(sl.w, i0, i1, i2, i3, i4, i5), A.box, A.periodic, v, rr,
                                          g0, g1, g2, g3);
                    }
                    if (publish) {
                        s_val[k * AMM_HB_LANES + lane] = v;
                        continue;
                    }
                    L.hot = k;
                    double e, de;
                    pexpr_run(s_code, ncode, s_consts, s_globals, L, s_stack + lane, e, de);
                    if (k == 0) e_sum += e;
                    if (k < V) {
                        const double coef = -de / rr;       // (rr = 1 but for a distance)
                        const int arity = cvar_arity(kind);
                        const int o0 = sl.x - base, o1 = arity > 1 ? sl.y - base : -1, o2 = arity > 2 ? sl.z - base : -1,
                                  o3 = arity > 3 ? sl.w - base : -1;
#pragma unroll
                        for (int x = 0; x < 3; ++x) {       // role by role, in role order
                            const double c0 = coef * g0[x], c1 = coef * g1[x], c2 = coef * g2[x], c3 = coef * g3[x];
                            if (o0 == 0) f0[x] += c0;
                            if (o0 == 1) f1[x] += c0;
                            if (o0 == 2) f2[x] += c0;
                            if (o1 == 0) f0[x] += c1;
                            if (o1 == 1) f1[x] += c1;
                            if (o1 == 2) f2[x] += c1;
                            if (o2 == 0) f0[x] += c2;
                            if (o2 == 1) f1[x] += c2;
                            if (o2 == 2) f2[x] += c2;
                            if (o3 == 0) f0[x] += c3;
                            if (o3 == 1) f1[x] += c3;
                            if (o3 == 2) f2[x] += c3;
                        }
                    }
                }
                ++n_pass;
            }
            qn = queue_keep_rest(s_queue, qn, take);        // what is left moves to the front
        }
        if (last) break;
    }
    for (int off = 32; off > 0; off >>= 1) {    // a fixed-order butterfly
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            f0[x] += __shfl_xor(f0[x], off);
            f1[x] += __shfl_xor(f1[x], off);
            f2[x] += __shfl_xor(f2[x], off);
        }
        if (EN) {
            e_sum += __shfl_xor(e_sum, off);
            n_pass += __shfl_xor(n_pass, off);
        }
    }
    if (lane == 0) {
        double *out = A.park + (size_t)blockIdx.x * 9;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            out[x] = f0[x];
            out[3 + x] = f1[x];
            out[6 + x] = f2[x];
        }
        if (EN) {
            A.epart[blockIdx.x] = e_sum;
            A.count[blockIdx.x] = n_pass;
        }
    }
}

// one lane per atom: its (donor, role) records, then its (acceptor, role) records, each over the row's chunks in chunk order
__global__ void __launch_bounds__(256) k_hbond_gather(int n, int D, int chunks0, int chunks1, size_t base1, const int *__restrict__ ref_ptr,
                                                       const int *__restrict__ rec_src, const double *__restrict__ park,
                                                       double *__restrict__ force, int accumulate) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    const int re = ref_ptr[i + 1];
    for (int r = ref_ptr[i]; r < re; ++r) {
        const int src = rec_src[r], rowg = src / 3, role = src - 3 * rowg;
        const bool donor = rowg < D;
        const int chunks = donor ? chunks0 : chunks1;
        const double *p = park + ((donor ? (size_t)rowg * chunks0 : base1 + (size_t)(rowg - D) * chunks1) * 9 + 3 * role);
        for (int c = 0; c < chunks; ++c, p += 9) {
            f0 += p[0];
            f1 += p[1];
            f2 += p[2];
        }
    }
    store_force_row(force, i, f0, f1, f2, accumulate);
}

template <bool EN>
static void hb_launch(amm_ctx *ctx, HbondForce *hb, const HbondArgs &A, int blocks) {
    if (hb->compact) hipLaunchKernelGGL((k_hbond<EN, true>), dim3(blocks), dim3(AMM_HB_LANES), 0, ctx->stream, A, hb->prog.d, hb->d_tab);
    else hipLaunchKernelGGL((k_hbond<EN, false>), dim3(blocks), dim3(AMM_HB_LANES), 0, ctx->stream, A, hb->prog.d, hb->d_tab);
}

int amm_hbond_eval_impl(amm_ctx *ctx, HbondForce *hb, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    const bool pairs = hb->D > 0 && hb->A > 0;
    if (pairs) {
        // (the box may have changed since creation: a barostat)
        if (hb->periodic && hb->cutoff && !amm_cutoff_fits_box(ctx, hb->rc, "hydrogen-bond force (AMM_FORCE_HBOND)")) return 1;
        for (int p = 0; p < 2; ++p) {
            const HbondPass &P = hb->pass[p];
            HbondArgs A;
            A.pass = p;
            A.n_rows = P.n_rows;
            A.n_cols = P.n_cols;
            A.chunks = P.chunks;
            A.chunk_len = P.chunk_len;
            A.n_vars = hb->n_vars;
            A.periodic = hb->periodic;
            A.cutoff = hb->cutoff;
            A.n_dp = hb->n_dp;
            A.D = hb->D;
            A.A = hb->A;
            A.donors = hb->d_donors;
            A.acceptors = hb->d_acceptors;
            A.dpar = hb->d_dpar;
            A.apar = hb->d_apar;
            A.ex_ptr = P.d_ex_ptr;
            A.ex_col = P.d_ex_col;
            A.pos = d_pos;
            A.rc2 = hb->rc * hb->rc;
            A.park = hb->d_park + P.park_base * 9;
            A.epart = hb->d_epart;
            A.count = hb->d_count;
            A.box = ctx->box;
            const int blocks = P.n_rows * P.chunks;
            // (the donor pass always counts its survivors and sums the energy: amm_hbond_stats reads the count; the forces are the same bits)
            if (p == 0) hb_launch<true>(ctx, hb, A, blocks);
            else hb_launch<false>(ctx, hb, A, blocks);
            AMM_HIP(hipGetLastError());
            hb->launches++;
        }
        hb->evaluated = true;
    }
    // (a force without pairs still writes its rows: it may be the first member of its group)
    hipLaunchKernelGGL(k_hbond_gather, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, ctx->stream, n, hb->D, hb->pass[0].chunks, hb->pass[1].chunks,
                       hb->pass[1].park_base, hb->d_ref_ptr, hb->d_rec_src, hb->d_park, d_force, accumulate);
    AMM_HIP(hipGetLastError());
    hb->launches++;
    if (d_energy && pairs) return amm_reduce_add(ctx, hb->d_epart, hb->pass[0].n_rows * hb->pass[0].chunks, 1.0, d_energy);
    return 0;
}

// ---- host ----
int amm_hbond_create_impl(amm_ctx *ctx, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals, int nglobal,
                          const int32_t *var_kinds, const int32_t *var_slots, int n_vars, const int32_t *h_donors, int n_donors,
                          const int32_t *h_acceptors, int n_acceptors, const double *h_dpar, int n_dpar, const double *h_apar, int n_apar,
                          const int32_t *h_excl, int n_excl, double rc, int periodic, HbondForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_hbond_create: " + what);
        return 1;
    };
    const int n = ctx->n, D = n_donors, A = n_acceptors;
    if (ctx->world > 1) return fail("a hydrogen-bond force (AMM_FORCE_HBOND) runs on a single rank");
    if (D < 0 || A < 0 || n_excl < 0) return fail("a negative count");
    if (D > AMM_HB_MAX_ROWS) return fail(std::to_string(D) + " donors (limit " + std::to_string(AMM_HB_MAX_ROWS) + ")");
    if (A > AMM_HB_MAX_ROWS) return fail(std::to_string(A) + " acceptors (limit " + std::to_string(AMM_HB_MAX_ROWS) + ")");
    if (n_vars < 0 || n_vars > AMM_COMPOUND_MAX_VARS) return fail(std::to_string(n_vars) + " geometric variables (limit " + std::to_string(AMM_COMPOUND_MAX_VARS) + ")");
    if (n_dpar < 0 || n_apar < 0 || n_dpar + n_apar > AMM_TERM_MAX_PARAMS)
        return fail(std::to_string(n_dpar) + " per-donor and " + std::to_string(n_apar) + " per-acceptor parameters (limit " +
                    std::to_string(AMM_TERM_MAX_PARAMS) + " together)");
    if ((n_dpar > 0 && D > 0 && !h_dpar) || (n_apar > 0 && A > 0 && !h_apar)) return fail("null parameter array");
    if (!std::isfinite(rc)) return fail("the cutoff is not finite");
    if (periodic && !(rc > 0.0)) return fail("CutoffPeriodic needs a cutoff distance above zero");
    if (periodic && !ctx->has_box) return fail("CutoffPeriodic, but the context has no periodic box");
    if (periodic && !amm_cutoff_fits_box(ctx, rc, "amm_hbond_create")) return 1;
    bool used[6] = {false, false, false, false, false, false};
    VarTable tab;
    if (var_table_fill("amm_hbond_create", var_kinds, var_slots, n_vars, 6, AMM_CVAR_DISTANCE, "the kind ",
                       " (a hydrogen-bond text reads distance, angle and dihedral only)", "beyond the pair (6 slots: d1 d2 d3 a1 a2 a3)", tab, used))
        return 1;
    if (amm_expr_program_validate("amm_hbond_create", code, ncode, nconst, nglobal, n_vars, n_dpar + n_apar)) return 1;
    static const char *slot_name[6] = {"d1", "d2", "d3", "a1", "a2", "a3"};
    for (int side = 0; side < 2; ++side) {
        const int32_t *idx = side ? h_acceptors : h_donors;
        const int count = side ? A : D;
        const char *who = side ? "acceptor" : "donor";
        for (int t = 0; t < count; ++t)
            for (int r = 0; r < 3; ++r) {
                const int a = idx[3 * t + r];
                if (a >= n || a < -1 || (a == -1 && r == 0))
                    return fail("atom index " + std::to_string(a) + " of " + who + " " + std::to_string(t) + " is out of range");
                if (a == -1 && used[3 * side + r])
                    return fail(std::string("the text names ") + slot_name[3 * side + r] + ", which " + who + " " + std::to_string(t) + " leaves at -1");
            }
    }
    std::vector<std::pair<int, int>> ex(n_excl);
    for (int e = 0; e < n_excl; ++e) {
        const int d = h_excl[2 * e], a = h_excl[2 * e + 1];
        if (d < 0 || d >= D || a < 0 || a >= A)
            return fail("exclusion " + std::to_string(e) + " (donor " + std::to_string(d) + ", acceptor " + std::to_string(a) + ") is out of range");
        ex[e] = {d, a};
    }
    AMM_HIP(hipSetDevice(ctx->device));
    HbondForce *hb = new HbondForce();
    hb->D = D;
    hb->A = A;
    hb->n_vars = n_vars;
    hb->n_dp = n_dpar;
    hb->n_ap = n_apar;
    hb->periodic = periodic ? 1 : 0;
    hb->cutoff = rc > 0.0 ? 1 : 0;
    hb->rc = rc > 0.0 ? rc : 0.0;
    hb->compact = ctx->opt_hbond_compact;
    hb->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    // the passes: a row is split into chunks of columns (a multiple of 64 each) when there are few rows -- option hbond_chunks, or
    // enough wavefronts to fill the device
    for (int p = 0; p < 2; ++p) {
        HbondPass &P = hb->pass[p];
        P.n_rows = p ? A : D;
        P.n_cols = p ? D : A;
        const int batches = std::max(1, (P.n_cols + AMM_HB_LANES - 1) / AMM_HB_LANES);
        int want = ctx->opt_hbond_chunks > 0 ? ctx->opt_hbond_chunks : (4096 + std::max(P.n_rows, 1) - 1) / std::max(P.n_rows, 1);
        want = std::max(1, std::min(want, batches));
        const int per = (batches + want - 1) / want;
        P.chunk_len = per * AMM_HB_LANES;
        P.chunks = (batches + per - 1) / per;
    }
    hb->pass[0].park_base = 0;
    hb->pass[1].park_base = (size_t)D * hb->pass[0].chunks;
    const size_t records = hb->pass[1].park_base + (size_t)A * hb->pass[1].chunks;
    // the exclusions per row: a donor's acceptors ascending, then (the pairs turned round) an acceptor's donors ascending
    std::vector<int> ptr0, col0, ptr1, col1;
    csr_of_pairs(D, ex, ptr0, col0);
    for (auto &e : ex) std::swap(e.first, e.second);
    csr_of_pairs(A, ex, ptr1, col1);
    // CSR of the records per atom: donors in index order, role by role, then acceptors
    std::vector<int> ptr, src;
    csr_of_records(n, [&](auto &&visit) {
        for (int t = 0; t < D; ++t)
            for (int r = 0; r < 3; ++r)
                if (h_donors[3 * t + r] >= 0) visit(h_donors[3 * t + r], t * 3 + r);
        for (int t = 0; t < A; ++t)
            for (int r = 0; r < 3; ++r)
                if (h_acceptors[3 * t + r] >= 0) visit(h_acceptors[3 * t + r], (D + t) * 3 + r);
    }, ptr, src);
    auto alloc = [&]() {
        if (hb->prog.upload(ctx, false)) return 1;
        if (amm_upload(&hb->d_tab, &tab, 1)) return 1;
        if (amm_upload(&hb->d_donors, h_donors, (size_t)D * 3)) return 1;
        if (amm_upload(&hb->d_acceptors, h_acceptors, (size_t)A * 3)) return 1;
        if (amm_upload(&hb->d_dpar, h_dpar, (size_t)D * n_dpar)) return 1;
        if (amm_upload(&hb->d_apar, h_apar, (size_t)A * n_apar)) return 1;
        if (amm_upload(&hb->pass[0].d_ex_ptr, ptr0.data(), ptr0.size())) return 1;
        if (amm_upload(&hb->pass[0].d_ex_col, col0.data(), col0.size())) return 1;
        if (amm_upload(&hb->pass[1].d_ex_ptr, ptr1.data(), ptr1.size())) return 1;
        if (amm_upload(&hb->pass[1].d_ex_col, col1.data(), col1.size())) return 1;
        if (amm_upload(&hb->d_ref_ptr, ptr.data(), ptr.size())) return 1;
        if (amm_upload(&hb->d_rec_src, src.data(), src.size())) return 1;
        const size_t park = std::max<size_t>(records * 9, 1), parts = std::max<size_t>((size_t)D * hb->pass[0].chunks, 1);
        AMM_HIP(hipMalloc(&hb->d_park, sizeof(double) * park));
        AMM_HIP(hipMemset(hb->d_park, 0, sizeof(double) * park));
        AMM_HIP(hipMalloc(&hb->d_epart, sizeof(double) * parts));
        AMM_HIP(hipMalloc(&hb->d_count, sizeof(int) * parts));
        AMM_HIP(hipMemset(hb->d_count, 0, sizeof(int) * parts));
        return 0;
    };
    if (alloc()) {
        amm_hbond_free(hb);
        return 1;
    }
    *out = hb;
    return 0;
}

int amm_hbond_set_globals_impl(amm_ctx *ctx, HbondForce *hb, const double *globals, int nglobal) {
    return hb->prog.set_globals(ctx, "amm_hbond_set_globals", globals, nglobal);
}

int amm_hbond_set_params_impl(amm_ctx *ctx, HbondForce *hb, const double *h_dpar, int n_donors, int n_dpar, const double *h_apar, int n_acceptors,
                              int n_apar) {
    const size_t nd = (size_t)hb->D * hb->n_dp, na = (size_t)hb->A * hb->n_ap;
    if (n_donors != hb->D || n_dpar != hb->n_dp || n_acceptors != hb->A || n_apar != hb->n_ap || (nd > 0 && !h_dpar) || (na > 0 && !h_apar)) {
        amm_set_error("amm_hbond_set_params: the force has " + std::to_string(hb->D) + " donors of " + std::to_string(hb->n_dp) + " parameters and " +
                      std::to_string(hb->A) + " acceptors of " + std::to_string(hb->n_ap) + ", " + std::to_string(n_donors) + " x " +
                      std::to_string(n_dpar) + " and " + std::to_string(n_acceptors) + " x " + std::to_string(n_apar) + " given");
        return 1;
    }
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (nd) AMM_HIP(hipMemcpy(hb->d_dpar, h_dpar, sizeof(double) * nd, hipMemcpyHostToDevice));
    if (na) AMM_HIP(hipMemcpy(hb->d_apar, h_apar, sizeof(double) * na, hipMemcpyHostToDevice));
    return 0;
}

// out[0]: ordered pairs one pass scans (D x A); out[1]: those that passed the cutoff and the exclusions in the last evaluation;
// out[2]: launches so far; out[3]: chunks per donor row
int amm_hbond_stats_impl(amm_ctx *ctx, HbondForce *hb, int64_t out[4]) {
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t parts = (size_t)hb->D * hb->pass[0].chunks;
    long long kept = 0;
    if (hb->evaluated && parts) {
        std::vector<int> count(parts);
        AMM_HIP(hipMemcpy(count.data(), hb->d_count, sizeof(int) * parts, hipMemcpyDeviceToHost));
        for (int c : count) kept += c;
    }
    out[0] = (int64_t)hb->D * hb->A;
    out[1] = kept;
    out[2] = hb->launches;
    out[3] = hb->pass[0].chunks;
    return 0;
}

void amm_hbond_free(HbondForce *hb) {
    if (!hb) return;
    for (void *p : {(void *)hb->prog.d, (void *)hb->d_tab, (void *)hb->d_donors, (void *)hb->d_acceptors, (void *)hb->d_dpar, (void *)hb->d_apar,
                    (void *)hb->pass[0].d_ex_ptr, (void *)hb->pass[0].d_ex_col, (void *)hb->pass[1].d_ex_ptr, (void *)hb->pass[1].d_ex_col,
                    (void *)hb->d_park, (void *)hb->d_epart, (void *)hb->d_count, (void *)hb->d_ref_ptr, (void *)hb->d_rec_src})
        if (p) (void)hipFree(p);
    delete hb;
}
