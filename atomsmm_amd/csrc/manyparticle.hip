// atomsmm_amd/csrc/manyparticle.hip -- CustomManyParticleForce with ANY energy text over sets of THREE particles
// (AMM_FORCE_MANY_PARTICLE): every set {i, j, k} of distinct particles no pair of which is excluded and which lies inside the cutoff
// contributes the text -- up to 16 geometric variables distance / angle / dihedral / raw coordinates over p1 p2 p3, per-particle
// parameters suffixed with the role, global parameters -- compiled by atomsmm_amd/expr.py (compile_many_particle) into the program
// of pair_expr_vm.h plus the variable table of expr_force.h (slots 0 .. 2 = p1 p2 p3).  DESIGN.md 3.MP has the semantics.
//
// Two launches per evaluation, one wavefront (a block of 64 lanes) per particle in both:
//  k_many_neighbors  row i scans all columns 64 at a time -- j != i, inside the cutoff (the displacement taken as lower index minus
//                    higher index, so rows i and j test the same number), not in row i's sorted exclusion list -- and appends the
//                    survivors in ascending order with ballot + prefix count to row i of a table [n][capacity].  The row's true
//                    count is stored unclamped; a row that needs more than the capacity is clamped in the table and raises a flag by
//                    a plain store, which amm_check reports by name.
//  k_many            owner computes: the wavefront of particle i enumerates every set that contains i -- SinglePermutation: the
//                    pairs (j < k) of nbr(i) with |x_j - x_k| inside the cutoff and (j, k) not excluded; UniqueCentralParticle: i as
//                    the centre over the pairs (j < k) of nbr(i) with (j, k) not excluded, then i as a satellite over c in nbr(i)
//                    and k in nbr(c), k != i, (i, k) not excluded -- 64 candidates at a time.  The survivors queue in LDS as the
//                    atoms of p1 p2 p3 (the permutation of the type table applied) and the owner's role; the interpreter runs on
//                    full queues and once at the end of the row, as k_hbond does: a draining lane computes the V variables
//                    (compound_geom.h), runs pexpr_run once per variable with a one-hot seed and adds -dE/dv grad v of the OWNER's
//                    role to three register accumulators.  A fixed-order butterfly sums the lanes and lane 0 adds the row's sum to
//                    f[i]: no parking and no gather.  The energy is summed by the owner with the lowest index (single mode) or by
//                    the centre (central mode) and reduced in row order.
// So every set is interpreted three times, once per owner.
//
// No atomics, fp contraction off, all fp64; one instantiation serves evaluations with and without energy: the same positions give
// the same bits.  No dynamically indexed private array of this file's own.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "compound_geom.h"
#include "device_utils.h"
#include "term_expr_vm.h"

#define AMM_MP_LANES 64
#define AMM_MP_MAX_PARTICLES 32768
#define AMM_MP_MAX_NOCUTOFF 2048
#define AMM_MP_MAX_TYPES 16
#define AMM_MP_MAX_PARAMS 2

struct ManyForce {
    int n = 0, n_vars = 0, n_par = 0, n_types = 1, periodic = 0, cutoff = 0, central = 0, capacity = 64;
    double rc = 0.0;
    ExprProgram prog;
    VarTable *d_tab = nullptr;
    double *d_par = nullptr;            // [n_par][n]
    int *d_type = nullptr;              // [n] dense type indices
    int *d_perm = nullptr;              // [T][T][T] permutation code 0 .. 5 of the tuple's types, -1: the set is skipped
    int *d_ex_ptr = nullptr, *d_ex_col = nullptr;   // CSR of a particle's excluded partners, sorted (both directions)
    int *d_nbr = nullptr;               // [n][capacity]
    int *d_nbr_count = nullptr;         // [n] unclamped
    int *d_flag = nullptr;              // [1] a row needed more than the capacity
    double *d_epart = nullptr;          // [n]
    int *d_sets = nullptr;              // [n] sets whose energy row i summed in the last evaluation
    long long launches = 0;
    bool evaluated = false;
};

// The leaves of a many-particle text: variable k is TERM_VAR k, read from the lane's own row of values in LDS; the seed is the
// one-hot of this run; parameter k is per-particle parameter k % P of the particle in role k / P, read parameter-major.
struct ManyLeaves {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_MP_LANES;
    const double *vars;
    int hot, n_par, a0, a1, a2;
    const double *par;
    size_t n;
    __device__ __forceinline__ double var(int k) const { return vars[k * AMM_MP_LANES]; }
    __device__ __forceinline__ double seed(int k) const { return k == hot ? 1.0 : 0.0; }
    __device__ __forceinline__ double param(int k) const {
        const int r = n_par == 2 ? k >> 1 : k, p = n_par == 2 ? k & 1 : 0;
        return par[(size_t)p * n + (r == 0 ? a0 : (r == 1 ? a1 : a2))];
    }
};

struct ManyArgs {
    int n, n_vars, n_par, n_types, periodic, cutoff, central, capacity;
    const double *par;
    const int *type, *perm;
    const int *ex_ptr, *ex_col;
    int *nbr, *nbr_count, *flag;
    const double *pos;
    double rc2;
    double *force;
    int accumulate;
    double *epart;
    int *sets;
    Box box;
};

// |x_a - x_b|^2 with a < b (lower index minus higher index: every wavefront that tests the pair tests the same number)
__device__ __forceinline__ double mp_dist2(const double *__restrict__ pos, int a, int b, const Box &box, int periodic) {
#pragma clang fp contract(off)
    const int lo = min(a, b), hi = max(a, b);
    double dx = pos[3 * lo] - pos[3 * hi], dy = pos[3 * lo + 1] - pos[3 * hi + 1], dz = pos[3 * lo + 2] - pos[3 * hi + 2];
    if (periodic) {
        dx = amm_min_image(dx, box.L[0], box.invL[0]);
        dy = amm_min_image(dy, box.L[1], box.invL[1]);
        dz = amm_min_image(dz, box.L[2], box.invL[2]);
    }
    return dx * dx + dy * dy + dz * dz;
}

__global__ void __launch_bounds__(AMM_MP_LANES) k_many_neighbors(ManyArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, i = blockIdx.x;       // (the grid is n)
    const int ex_begin = A.ex_ptr[i], ex_end = A.ex_ptr[i + 1];
    int *row = A.nbr + (size_t)i * A.capacity;
    int count = 0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_MP_LANES) {
        const int col = j0 + lane;
        bool keep = col < A.n && col != i;
        if (keep && A.cutoff) keep = mp_dist2(A.pos, i, col, A.box, A.periodic) < A.rc2;
        if (keep && ex_end > ex_begin) keep = !sorted_contains(A.ex_col, ex_begin, ex_end, col);
        const unsigned long long mask = __ballot(keep);
        const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && at < A.capacity) row[at] = col;
        count += __popcll(mask);
    }
    if (lane == 0) {
        A.nbr_count[i] = count;
        if (count > A.capacity) A.flag[0] = 1;          // (a plain store: every writer writes the same value)
    }
}

__device__ __forceinline__ int mp_pick(int s, int i0, int i1, int i2) { return s == 0 ? i0 : (s == 1 ? i1 : i2); }

// The atoms of p1 p2 p3 from the tuple (t0, t1, t2) and the code of the permutation (lexicographic over the tuple's positions):
// role r is played by the tuple's element perm[r].
__device__ __forceinline__ void mp_permute(int code, int t0, int t1, int t2, int &p1, int &p2, int &p3) {
    const int e0 = code >> 1;                                       // 0 0 1 1 2 2
    const int e1 = code == 0 ? 1 : (code == 1 ? 2 : (code == 2 ? 0 : (code == 3 ? 2 : (code == 4 ? 0 : 1))));
    const int e2 = 3 - e0 - e1;
    p1 = mp_pick(e0, t0, t1, t2);
    p2 = mp_pick(e1, t0, t1, t2);
    p3 = mp_pick(e2, t0, t1, t2);
}

__global__ void __launch_bounds__(AMM_MP_LANES) k_many(ManyArgs A, const PairExprProg *__restrict__ prog, const VarTable *__restrict__ tab) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ int s_kind[AMM_COMPOUND_MAX_VARS];
    __shared__ int4 s_slot[AMM_COMPOUND_MAX_VARS];
    __shared__ double s_val[AMM_COMPOUND_MAX_VARS * AMM_MP_LANES];                 // value k of lane t: s_val[k * 64 + t]
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_MP_LANES];              // all but the top of every lane's stack
    __shared__ int4 s_queue[2 * AMM_MP_LANES];                                      // (p1, p2, p3, owner's role | energy << 2) that wait
    const int lane = threadIdx.x;
    const int ncode = prog->ncode;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    var_table_stage(tab, s_kind, s_slot);
    __syncthreads();
    const int i = blockIdx.x;                   // (the grid is n)
    const int cap = A.capacity, T = A.n_types;
    const int m = min(A.nbr_count[i], cap);
    const int *nb = A.nbr + (size_t)i * cap;
    const int ex_i0 = A.ex_ptr[i], ex_i1 = A.ex_ptr[i + 1];
    const int type_i = A.type[i];
    const PosPlain pos{A.pos};
    double fx = 0.0, fy = 0.0, fz = 0.0, e_sum = 0.0;
    int n_sets = 0, qn = 0;
    // part 0: the pairs (a < b) of nbr(i), numbered row by row of the triangle, 64 at a time; part 1 (central mode): for each
    // neighbour c, the members of nbr(c) 64 at a time.  `outer` and `inner` walk either.
    const long long n_pairs = (long long)m * (m - 1) / 2;
    int part = 0, outer = 0;
    long long inner = 0;
    for (;;) {
        // ---- what this turn tests (wave-uniform)
        bool last = false;
        if (part == 0 && inner >= n_pairs) {
            part = 1;
            outer = 0;
            inner = 0;
        }
        int c = -1, mc = 0;
        if (part == 1) {
            if (!A.central) last = true;
            else {
                while (outer < m) {
                    c = nb[outer];
                    mc = min(A.nbr_count[c], cap);
                    if (inner < mc) break;
                    ++outer;
                    inner = 0;
                }
                if (outer >= m) last = true;
            }
        }
        if (!last) {
            bool keep = false;
            int p1 = 0, p2 = 0, p3 = 0, meta = 0;
            if (part == 0) {
                const long long p = inner + lane;
                if (p < n_pairs) {
                    // row a of the triangle starts at a (2 m - a - 1) / 2
                    const double bq = (double)(2 * m - 1);
                    int a = (int)((bq - sqrt(bq * bq - 8.0 * (double)p)) * 0.5);
                    a = max(0, min(a, m - 2));
                    while (a > 0 && (long long)a * (2 * m - a - 1) / 2 > p) --a;
                    while (a < m - 2 && (long long)(a + 1) * (2 * m - a - 2) / 2 <= p) ++a;
                    const int b = a + 1 + (int)(p - (long long)a * (2 * m - a - 1) / 2);
                    const int j = nb[a], k = nb[b];         // j < k: the row ascends
                    keep = true;
                    if (!A.central && A.cutoff) keep = mp_dist2(A.pos, j, k, A.box, A.periodic) < A.rc2;
                    if (keep) {
                        const int lo = A.ex_ptr[j], hi = A.ex_ptr[j + 1];
                        if (hi > lo) keep = !sorted_contains(A.ex_col, lo, hi, k);
                    }
                    if (keep) {
                        int t0, t1, t2;
                        if (A.central) {                    // the centre first, the satellites ascending
                            t0 = i;
                            t1 = j;
                            t2 = k;
                        } else {                            // ascending
                            t0 = min(i, j);
                            t1 = i < j ? j : min(i, k);
                            t2 = max(i, k);
                        }
                        const int code = A.perm[(A.type[t0] * T + A.type[t1]) * T + A.type[t2]];
                        keep = code >= 0;
                        if (keep) {
                            mp_permute(code, t0, t1, t2, p1, p2, p3);
                            const int role = p1 == i ? 0 : (p2 == i ? 1 : 2);
                            meta = role | ((A.central || i < j) ? 4 : 0);
                        }
                    }
                }
                inner += AMM_MP_LANES;
            } else {
                const long long q = inner + lane;
                if (q < mc) {
                    const int k = A.nbr[(size_t)c * cap + (int)q];
                    keep = k != i;
                    if (keep && ex_i1 > ex_i0) keep = !sorted_contains(A.ex_col, ex_i0, ex_i1, k);
                    if (keep) {
                        const int t1 = min(i, k), t2 = max(i, k);
                        const int code = A.perm[(A.type[c] * T + (i < k ? type_i : A.type[k])) * T + (i < k ? A.type[k] : type_i)];
                        keep = code >= 0;
                        if (keep) {
                            mp_permute(code, c, t1, t2, p1, p2, p3);
                            meta = p1 == i ? 0 : (p2 == i ? 1 : 2);      // (the centre sums the energy)
                        }
                    }
                }
                inner += AMM_MP_LANES;
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) s_queue[qn + __popcll(mask & ((1ull << lane) - 1ull))] = make_int4(p1, p2, p3, meta);      // (qn < 64 here: at most 127 entries)
            qn += __popcll(mask);
            __syncthreads();
        }
        if (qn >= AMM_MP_LANES || (last && qn > 0)) {
            const int take = min(qn, AMM_MP_LANES);
            if (lane < take) {
                const int4 q = s_queue[lane];
                const int i0 = q.x, i1 = q.y, i2 = q.z, role = q.w & 3;
                ManyLeaves L;
                L.vars = s_val + lane;
                L.n_par = A.n_par;
                L.a0 = i0;
                L.a1 = i1;
                L.a2 = i2;
                L.par = A.par;
                L.n = (size_t)A.n;
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
                        compound_variable(pos, kind, mp_pick(sl.x, i0, i1, i2), mp_pick(sl.y, i0, i1, i2), mp_pick(sl.z, i0, i1, i2),
                                          mp_pick(sl.w, i0, i1, i2), A.box, A.periodic, v, rr, g0, g1, g2, g3);
                    }
                    if (publish) {
                        s_val[k * AMM_MP_LANES + lane] = v;
                        continue;
                    }
                    L.hot = k;
                    double e, de;
                    pexpr_run(s_code, ncode, s_consts, s_globals, L, s_stack + lane, e, de);
                    if (k == 0 && (q.w & 4)) {
                        e_sum += e;
                        ++n_sets;
                    }
                    if (k < V) {
                        const double coef = -de / rr;       // (rr = 1 but for a distance)
                        const int arity = cvar_arity(kind);
                        const bool o0 = sl.x == role, o1 = arity > 1 && sl.y == role, o2 = arity > 2 && sl.z == role, o3 = arity > 3 && sl.w == role;
                        if (o0) {
                            fx += coef * g0[0];
                            fy += coef * g0[1];
                            fz += coef * g0[2];
                        }
                        if (o1) {
                            fx += coef * g1[0];
                            fy += coef * g1[1];
                            fz += coef * g1[2];
                        }
                        if (o2) {
                            fx += coef * g2[0];
                            fy += coef * g2[1];
                            fz += coef * g2[2];
                        }
                        if (o3) {
                            fx += coef * g3[0];
                            fy += coef * g3[1];
                            fz += coef * g3[2];
                        }
                    }
                }
            }
            qn = queue_keep_rest(s_queue, qn, take);        // what is left moves to the front
        }
        if (last) break;
    }
    for (int off = 32; off > 0; off >>= 1) {    // a fixed-order butterfly
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
        e_sum += __shfl_xor(e_sum, off);
        n_sets += __shfl_xor(n_sets, off);
    }
    if (lane == 0) {
        store_force_row(A.force, i, fx, fy, fz, A.accumulate);
        A.epart[i] = e_sum;
        A.sets[i] = n_sets;
    }
}

// a force without particles still writes its rows: it may be the first member of its group
__global__ void __launch_bounds__(256) k_many_zero(int n3, double *__restrict__ force) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n3) force[t] = 0.0;
}

int amm_many_eval_impl(amm_ctx *ctx, ManyForce *mf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = mf->n;
    if (n == 0) {
        if (!accumulate && ctx->n > 0) {
            hipLaunchKernelGGL(k_many_zero, dim3((3 * ctx->n + 255) / 256), dim3(256), 0, ctx->stream, 3 * ctx->n, d_force);
            AMM_HIP(hipGetLastError());
        }
        return 0;
    }
    // the box may have changed since creation (a barostat)
    if (mf->periodic && mf->cutoff && !amm_cutoff_fits_box(ctx, mf->rc, "many-particle force (AMM_FORCE_MANY_PARTICLE)")) return 1;
    ManyArgs A;
    A.n = n;
    A.n_vars = mf->n_vars;
    A.n_par = mf->n_par;
    A.n_types = mf->n_types;
    A.periodic = mf->periodic;
    A.cutoff = mf->cutoff;
    A.central = mf->central;
    A.capacity = mf->capacity;
    A.par = mf->d_par;
    A.type = mf->d_type;
    A.perm = mf->d_perm;
    A.ex_ptr = mf->d_ex_ptr;
    A.ex_col = mf->d_ex_col;
    A.nbr = mf->d_nbr;
    A.nbr_count = mf->d_nbr_count;
    A.flag = mf->d_flag;
    A.pos = d_pos;
    A.rc2 = mf->rc * mf->rc;
    A.force = d_force;
    A.accumulate = accumulate;
    A.epart = mf->d_epart;
    A.sets = mf->d_sets;
    A.box = ctx->box;
    hipLaunchKernelGGL(k_many_neighbors, dim3(n), dim3(AMM_MP_LANES), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_many, dim3(n), dim3(AMM_MP_LANES), 0, ctx->stream, A, mf->prog.d, mf->d_tab);
    AMM_HIP(hipGetLastError());
    mf->launches += 2;
    mf->evaluated = true;
    if (d_energy) return amm_reduce_add(ctx, mf->d_epart, n, 1.0, d_energy);
    return 0;
}

// ---- host ----
// the types and the permutation table of a creation or an update; what names the caller
static int mp_check_types(const char *who, int n, const int32_t *h_types, int n_types, const int32_t *h_perm, int central) {
    auto fail = [&](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what);
        return 1;
    };
    if (n_types < 1 || n_types > AMM_MP_MAX_TYPES) return fail(std::to_string(n_types) + " particle types (limit " + std::to_string(AMM_MP_MAX_TYPES) + ")");
    for (int i = 0; i < n; ++i)
        if (h_types[i] < 0 || h_types[i] >= n_types)
            return fail("particle " + std::to_string(i) + " has the type index " + std::to_string(h_types[i]) + " (the force has " + std::to_string(n_types) + " types)");
    for (int t = 0; t < n_types * n_types * n_types; ++t)
        if (h_perm[t] < -1 || h_perm[t] > (central ? 1 : 5))
            return fail("entry " + std::to_string(t) + " of the permutation table is " + std::to_string(h_perm[t]) + " (-1: skip; 0 .. " + (central ? "1" : "5") + ")");
    return 0;
}

int amm_many_create_impl(amm_ctx *ctx, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals, int nglobal,
                         const int32_t *var_kinds, const int32_t *var_slots, int n_vars, int n_particles, const double *h_params, int n_params,
                         const int32_t *h_types, int n_types, const int32_t *h_perm, const int32_t *h_excl, int n_excl, double rc, int periodic,
                         int central, ManyForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_many_create: " + what);
        return 1;
    };
    const int n = n_particles;
    if (ctx->world > 1) return fail("a many-particle force (AMM_FORCE_MANY_PARTICLE) runs on a single rank");
    if (n < 0 || n_excl < 0) return fail("a negative count");
    if (n != 0 && n != ctx->n) return fail(std::to_string(n) + " particles, but the context has " + std::to_string(ctx->n) + " atoms");
    if (n > AMM_MP_MAX_PARTICLES) return fail(std::to_string(n) + " particles (limit " + std::to_string(AMM_MP_MAX_PARTICLES) + ")");
    if (!std::isfinite(rc)) return fail("the cutoff is not finite");
    if (!(rc > 0.0) && n > AMM_MP_MAX_NOCUTOFF)
        return fail(std::to_string(n) + " particles under NoCutoff (limit " + std::to_string(AMM_MP_MAX_NOCUTOFF) + ": the neighbour table is n x (n - 1))");
    if (n_vars < 0 || n_vars > AMM_COMPOUND_MAX_VARS) return fail(std::to_string(n_vars) + " geometric variables (limit " + std::to_string(AMM_COMPOUND_MAX_VARS) + ")");
    if (n_params < 0 || n_params > AMM_MP_MAX_PARAMS)
        return fail(std::to_string(n_params) + " per-particle parameters (limit " + std::to_string(AMM_MP_MAX_PARAMS) + ": three copies each)");
    if (n_params > 0 && n > 0 && !h_params) return fail("null parameter array");
    if (periodic && !(rc > 0.0)) return fail("CutoffPeriodic needs a cutoff distance above zero");
    if (periodic && !ctx->has_box) return fail("CutoffPeriodic, but the context has no periodic box");
    VarTable tab;
    if (var_table_fill("amm_many_create", var_kinds, var_slots, n_vars, 3, AMM_CVAR_X, "the kind ", "", "beyond the set (3 slots: p1 p2 p3)", tab, nullptr))
        return 1;
    if (amm_expr_program_validate("amm_many_create", code, ncode, nconst, nglobal, n_vars, 3 * n_params)) return 1;
    if (mp_check_types("amm_many_create", n, h_types, n_types, h_perm, central)) return 1;
    std::vector<std::pair<int, int>> ex;
    ex.reserve(2 * (size_t)n_excl);
    for (int e = 0; e < n_excl; ++e) {
        const int a = h_excl[2 * e], b = h_excl[2 * e + 1];
        if (a < 0 || a >= n || b < 0 || b >= n)
            return fail("exclusion " + std::to_string(e) + " (particles " + std::to_string(a) + ", " + std::to_string(b) + ") is out of range");
        if (a == b) continue;
        ex.push_back({a, b});
        ex.push_back({b, a});
    }
    AMM_HIP(hipSetDevice(ctx->device));
    ManyForce *mf = new ManyForce();
    mf->n = n;
    mf->n_vars = n_vars;
    mf->n_par = n_params;
    mf->n_types = n_types;
    mf->periodic = periodic ? 1 : 0;
    mf->cutoff = rc > 0.0 ? 1 : 0;
    mf->rc = rc > 0.0 ? rc : 0.0;
    mf->central = central ? 1 : 0;
    mf->capacity = mf->cutoff ? ctx->opt_many_capacity : std::max(64, (n - 1 + 63) / 64 * 64);
    if (mf->periodic && !amm_cutoff_fits_box(ctx, mf->rc, "amm_many_create")) {
        delete mf;
        return 1;
    }
    mf->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    std::vector<int> ptr, col;
    csr_of_pairs(n, ex, ptr, col);
    auto alloc = [&]() {
        if (mf->prog.upload(ctx, false)) return 1;
        if (amm_upload(&mf->d_tab, &tab, 1)) return 1;
        if (amm_upload(&mf->d_par, h_params, (size_t)n * n_params)) return 1;
        if (amm_upload(&mf->d_type, h_types, (size_t)n)) return 1;
        if (amm_upload(&mf->d_perm, h_perm, (size_t)n_types * n_types * n_types)) return 1;
        if (amm_upload(&mf->d_ex_ptr, ptr.data(), ptr.size())) return 1;
        if (amm_upload(&mf->d_ex_col, col.data(), col.size())) return 1;
        const size_t rows = std::max<size_t>(n, 1);
        AMM_HIP(hipMalloc(&mf->d_nbr, sizeof(int) * rows * mf->capacity));
        AMM_HIP(hipMemset(mf->d_nbr, 0, sizeof(int) * rows * mf->capacity));
        AMM_HIP(hipMalloc(&mf->d_nbr_count, sizeof(int) * rows));
        AMM_HIP(hipMemset(mf->d_nbr_count, 0, sizeof(int) * rows));
        AMM_HIP(hipMalloc(&mf->d_flag, sizeof(int)));
        AMM_HIP(hipMemset(mf->d_flag, 0, sizeof(int)));
        AMM_HIP(hipMalloc(&mf->d_epart, sizeof(double) * rows));
        AMM_HIP(hipMemset(mf->d_epart, 0, sizeof(double) * rows));
        AMM_HIP(hipMalloc(&mf->d_sets, sizeof(int) * rows));
        AMM_HIP(hipMemset(mf->d_sets, 0, sizeof(int) * rows));
        return 0;
    };
    if (alloc()) {
        amm_many_free(mf);
        return 1;
    }
    *out = mf;
    return 0;
}

int amm_many_set_globals_impl(amm_ctx *ctx, ManyForce *mf, const double *globals, int nglobal) {
    return mf->prog.set_globals(ctx, "amm_many_set_globals", globals, nglobal);
}

int amm_many_set_params_impl(amm_ctx *ctx, ManyForce *mf, const double *h_params, int n_particles, int n_params, const int32_t *h_types, int n_types,
                             const int32_t *h_perm) {
    const size_t np = (size_t)mf->n * mf->n_par;
    if (n_particles != mf->n || n_params != mf->n_par || (np > 0 && !h_params) || !h_types || !h_perm) {
        amm_set_error("amm_many_set_params: the force has " + std::to_string(mf->n) + " particles of " + std::to_string(mf->n_par) + " parameters, " +
                      std::to_string(n_particles) + " x " + std::to_string(n_params) + " given");
        return 1;
    }
    if (mp_check_types("amm_many_set_params", mf->n, h_types, n_types, h_perm, mf->central)) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (np) AMM_HIP(hipMemcpy(mf->d_par, h_params, sizeof(double) * np, hipMemcpyHostToDevice));
    if (mf->n) AMM_HIP(hipMemcpy(mf->d_type, h_types, sizeof(int) * mf->n, hipMemcpyHostToDevice));
    const size_t cells = (size_t)n_types * n_types * n_types;
    if (n_types != mf->n_types) {           // another number of types: the table has another size
        int *fresh = nullptr;
        if (amm_upload(&fresh, h_perm, cells)) return 1;
        (void)hipFree(mf->d_perm);
        mf->d_perm = fresh;
        mf->n_types = n_types;
    } else {
        AMM_HIP(hipMemcpy(mf->d_perm, h_perm, sizeof(int) * cells, hipMemcpyHostToDevice));
    }
    return 0;
}

// out[0]: particles; out[1]: evaluations of the text whose energy was summed in the last evaluation (SinglePermutation: the sets;
// UniqueCentralParticle: one per set and centre); out[2]: launches so far; out[3]: the fullest neighbour row of the last evaluation,
// unclamped; out[4]: the capacity of a row
int amm_many_stats_impl(amm_ctx *ctx, ManyForce *mf, int64_t out[5]) {
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    long long sets = 0;
    int fullest = 0;
    if (mf->evaluated && mf->n) {
        std::vector<int> count(mf->n);
        AMM_HIP(hipMemcpy(count.data(), mf->d_sets, sizeof(int) * mf->n, hipMemcpyDeviceToHost));
        for (int c : count) sets += c;
        AMM_HIP(hipMemcpy(count.data(), mf->d_nbr_count, sizeof(int) * mf->n, hipMemcpyDeviceToHost));
        for (int c : count) fullest = std::max(fullest, c);
    }
    out[0] = mf->n;
    out[1] = sets;
    out[2] = mf->launches;
    out[3] = fullest;
    out[4] = mf->capacity;
    return 0;
}

// amm_check (the stream has been waited for): 1 with *need and *capacity when a neighbour row overflowed, 0 when none did, -1 on a HIP error
int amm_many_overflow(ManyForce *mf, int *need, int *capacity) {
    int flag = 0;
    if (hipMemcpy(&flag, mf->d_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (!flag) return 0;
    std::vector<int> count(std::max(mf->n, 1), 0);
    if (mf->n && hipMemcpy(count.data(), mf->d_nbr_count, sizeof(int) * mf->n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    *need = *std::max_element(count.begin(), count.end());
    *capacity = mf->capacity;
    return 1;
}

void amm_many_free(ManyForce *mf) {
    if (!mf) return;
    for (void *p : {(void *)mf->prog.d, (void *)mf->d_tab, (void *)mf->d_par, (void *)mf->d_type, (void *)mf->d_perm, (void *)mf->d_ex_ptr,
                    (void *)mf->d_ex_col, (void *)mf->d_nbr, (void *)mf->d_nbr_count, (void *)mf->d_flag, (void *)mf->d_epart, (void *)mf->d_sets})
        if (p) (void)hipFree(p);
    delete mf;
}
