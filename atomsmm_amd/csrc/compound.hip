// atomsmm_amd/csrc/compound.hip -- CustomCompoundBondForce and CustomCentroidBondForce with ANY energy text (AMM_FORCE_COMPOUND): a
// bond is N particles (or N weighted centres of groups of atoms) and its text reads up to 16 geometric variables over them --
// raw coordinates, distance(pa,pb), angle(pa,pb,pc), dihedral(pa,pb,pc,pd) -- compiled by atomsmm_amd/expr.py (compile_compound)
// into the program of pair_expr_vm.h plus a variable table (kind, slots within the bond: VarTable, expr_force.h).
//
// Takes over what OpenMM does for these two classes: per bond, the variables, the energy expression at them and its partial
// derivatives (Lepton differentiates the text; here the interpreter carries one derivative along per lane), and
// -sum_k dE/dv_k grad v_k on the particles.  The geometry is that of k_term_expr (term_expr.hip): delta3 / cross3 / amm_min_image of
// bonded_terms.h, the angle gradient with its 1 - c^2 floor, the dihedral convention and gradient of AMM_TORSION_PERIODIC.
//
// These forces have few bonds (one to a few hundred restraints): latency counts, not throughput.  So the scheme is k_cv_apply's,
// ONE LANE PER (BOND, VARIABLE): a bond takes L = the next power of two >= V lanes (1 .. 16; it never straddles a wavefront), lane k
// computes variable k and its gradient on at most four slots, publishes the value in the bond's row in LDS, and after the barrier
// runs pexpr_run seeded one-hot in k, which leaves dE/dv_k; it parks -dE/dv_k grad v_k of its slots (twelve doubles per (bond,
// variable)).  Lane 0 of a bond contributes the energy; the block reduction is k_term_expr's.  k_compound_gather, one lane per atom,
// adds the atom's (bond, variable, role) records in record order from a CSR built at creation and writes every row when it does
// not accumulate.
//
// Centres (CustomCentroidBondForce): k_compound_centres runs ahead, one wavefront per group -- members in lane-strided order, a
// fixed-order butterfly for the total weight and the weighted sum of RAW positions -- and the evaluation reads centres instead of
// atoms.  k_compound_spread, one lane per atom, walks the atom's memberships in group order, sums each group's records in record order
// and adds (w_i / W_g) times that sum.
//
// No atomics, fp contraction off: the same bits run to run, and the energy and the force-only instantiation give the same forces.
// No dynamically indexed private array of this file's own: the variable table is read from LDS and every gradient has static indices.
// DESIGN.md 3.CB has the resource figures and the measured cost.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "compound_geom.h"
#include "device_utils.h"
#include "term_expr_vm.h"

#define AMM_CB_BLOCK 256

struct CompoundForce {
    int n_slots = 0, n_vars = 0, shift = 0, n_bonds = 0, n_params = 0, periodic = 0, n_blocks = 1;
    int n_groups = 0, n_members = 0;    // n_groups > 0: the slots of a bond are groups (centroid bonds)
    ExprProgram prog;
    VarTable *d_tab = nullptr;
    int *d_idx = nullptr;               // [n_bonds][n_slots] atoms, or groups
    double *d_params = nullptr;         // [n_params][n_bonds]
    double *d_park = nullptr;           // [n_bonds][n_vars][4][3] parked forces of the variables' roles
    double *d_epart = nullptr;          // [n_blocks]
    int *d_ref_ptr = nullptr;           // [n + 1] (atoms) or [n_groups + 1] (groups): CSR of the (bond, variable, role) records ...
    int *d_rec_src = nullptr;           // ... each (bond * n_vars + variable) * 4 + role, in that order
    // centroid bonds only
    int *d_g_ptr = nullptr, *d_g_atom = nullptr;        // [n_groups + 1], [n_members]: members of a group
    double *d_g_w = nullptr;                            // [n_members] their weights
    double *d_centre = nullptr, *d_W = nullptr;         // [n_groups][3], [n_groups]
    int *d_a_ptr = nullptr, *d_a_grp = nullptr;         // [n + 1], [n_members]: memberships of an atom, in group order
    double *d_a_w = nullptr;                            // [n_members] the atom's weight in that group
    std::vector<int> a_member;                          // membership -> position in the groups' member list
};

// The leaves of a compound text: variable k is TERM_VAR k, read from the bond's row of published values; the seed is this lane's
// one-hot; parameter k is read parameter-major from global memory when the program asks for it.
struct CompoundLeaves {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_PEXPR_STRIDE;
    const double *vars;
    int lane;
    const double *p;
    size_t stride;
    __device__ __forceinline__ double var(int k) const { return vars[k]; }
    __device__ __forceinline__ double seed(int k) const { return k == lane ? 1.0 : 0.0; }
    __device__ __forceinline__ double param(int k) const { return p[(size_t)k * stride]; }
};

struct CompoundArgs {
    int n_bonds, n_slots, n_vars, shift, periodic;
    const int *idx;
    const double *params;
    const double *pos;          // atoms, or centres
    double *park;
    double *epart;
    Box box;
};

template <bool EN>
__global__ void __launch_bounds__(AMM_CB_BLOCK) k_compound(CompoundArgs A, const PairExprProg *__restrict__ prog,
                                                           const VarTable *__restrict__ tab) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ double s_val[AMM_CB_BLOCK];                                      // row of bond b: s_val[b << shift .. ]
    __shared__ int s_kind[AMM_COMPOUND_MAX_VARS];
    __shared__ int4 s_slot[AMM_COMPOUND_MAX_VARS];
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_PEXPR_STRIDE];      // all but the top of every lane's stack
    const int ncode = prog->ncode;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    var_table_stage(tab, s_kind, s_slot);
    __syncthreads();
    const int k = threadIdx.x & ((1 << A.shift) - 1);
    const int bond = blockIdx.x * (AMM_CB_BLOCK >> A.shift) + (threadIdx.x >> A.shift);
    const bool geo = bond < A.n_bonds && k < A.n_vars;
    const bool active = geo || (bond < A.n_bonds && k == 0);        // (a text without variables still has an energy)
    double v = 0.0, rr = 1.0;
    double g0[3] = {0.0, 0.0, 0.0}, g1[3] = {0.0, 0.0, 0.0}, g2[3] = {0.0, 0.0, 0.0}, g3[3] = {0.0, 0.0, 0.0};     // grad v on its roles
    int kind = 0;
    if (geo) {
        kind = s_kind[k];
        const int4 sl = s_slot[k];
        const int *ix = A.idx + (size_t)bond * A.n_slots;
        const PosPlain pos{A.pos};
        compound_variable(pos, kind, ix[sl.x], ix[sl.y], ix[sl.z], ix[sl.w], A.box, A.periodic, v, rr, g0, g1, g2, g3);     // compound_geom.h
    }
    s_val[threadIdx.x] = v;
    __syncthreads();
    double e = 0.0;
    if (active) {
        CompoundLeaves L;
        L.vars = s_val + (threadIdx.x - k);
        L.lane = k;
        L.p = A.params + bond;
        L.stride = (size_t)A.n_bonds;
        double de;
        pexpr_run(s_code, ncode, s_consts, s_globals, L, s_stack + threadIdx.x, e, de);
        if (geo) {
            const double coef = -de / rr;       // (rr = 1 but for a distance)
            double *out = A.park + ((size_t)bond * A.n_vars + k) * 12;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                out[x] = coef * g0[x];
                if (kind >= AMM_CVAR_DISTANCE) out[3 + x] = coef * g1[x];
                if (kind >= AMM_CVAR_ANGLE) out[6 + x] = coef * g2[x];
                if (kind == AMM_CVAR_DIHEDRAL) out[9 + x] = coef * g3[x];
            }
        }
        if (k != 0) e = 0.0;
    }
    if (EN) block_energy_store_256(e, A.epart);
}

// one lane per atom: its records, in record order (k_term_expr_gather's loop)
__global__ void __launch_bounds__(256) k_compound_gather(int n, const int *__restrict__ ref_ptr, const int *__restrict__ rec_src,
                                                         const double *__restrict__ park, double *__restrict__ force, int accumulate) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    const int re = ref_ptr[i + 1];
    for (int r = ref_ptr[i]; r < re; ++r) {
        const double *p = park + (size_t)rec_src[r] * 3;
        f0 += p[0];
        f1 += p[1];
        f2 += p[2];
    }
    store_force_row(force, i, f0, f1, f2, accumulate);
}

// one wavefront per group: W = sum w_i and sum w_i x_i over the raw positions, members lane-strided, then a fixed-order butterfly
__global__ void __launch_bounds__(256) k_compound_centres(int n_groups, const int *__restrict__ g_ptr, const int *__restrict__ g_atom,
                                                          const double *__restrict__ g_w, const double *__restrict__ pos,
                                                          double *__restrict__ centre, double *__restrict__ W) {
#pragma clang fp contract(off)
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= n_groups) return;          // (wave-uniform)
    double w = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    const int me = g_ptr[g + 1];
    for (int m = g_ptr[g] + lane; m < me; m += 64) {
        const int a = g_atom[m];
        const double ww = g_w[m];
        w += ww;
        sx += ww * pos[3 * a];
        sy += ww * pos[3 * a + 1];
        sz += ww * pos[3 * a + 2];
    }
    for (int off = 32; off > 0; off >>= 1) {
        w += __shfl_xor(w, off);
        sx += __shfl_xor(sx, off);
        sy += __shfl_xor(sy, off);
        sz += __shfl_xor(sz, off);
    }
    if (lane == 0) {
        centre[3 * g] = sx / w;
        centre[3 * g + 1] = sy / w;
        centre[3 * g + 2] = sz / w;
        W[g] = w;
    }
}

// one lane per atom: its memberships in group order; per group the sum of the group's records in record order, times w_i / W_g
__global__ void __launch_bounds__(256) k_compound_spread(int n, const int *__restrict__ a_ptr, const int *__restrict__ a_grp,
                                                         const double *__restrict__ a_w, const double *__restrict__ W,
                                                         const int *__restrict__ ref_ptr, const int *__restrict__ rec_src,
                                                         const double *__restrict__ park, double *__restrict__ force, int accumulate) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    const int me = a_ptr[i + 1];
    for (int m = a_ptr[i]; m < me; ++m) {
        const int g = a_grp[m];
        double F0 = 0.0, F1 = 0.0, F2 = 0.0;
        const int re = ref_ptr[g + 1];
        for (int r = ref_ptr[g]; r < re; ++r) {
            const double *p = park + (size_t)rec_src[r] * 3;
            F0 += p[0];
            F1 += p[1];
            F2 += p[2];
        }
        const double s = a_w[m] / W[g];
        f0 += s * F0;
        f1 += s * F1;
        f2 += s * F2;
    }
    store_force_row(force, i, f0, f1, f2, accumulate);
}

int amm_compound_eval_impl(amm_ctx *ctx, CompoundForce *cf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    const bool centroid = cf->n_groups > 0;
    if (centroid) {
        hipLaunchKernelGGL(k_compound_centres, dim3((cf->n_groups + 3) / 4), dim3(256), 0, ctx->stream, cf->n_groups, cf->d_g_ptr, cf->d_g_atom,
                           cf->d_g_w, d_pos, cf->d_centre, cf->d_W);
        AMM_HIP(hipGetLastError());
    }
    if (cf->n_bonds > 0) {
        CompoundArgs A;
        A.n_bonds = cf->n_bonds;
        A.n_slots = cf->n_slots;
        A.n_vars = cf->n_vars;
        A.shift = cf->shift;
        A.periodic = cf->periodic;
        A.idx = cf->d_idx;
        A.params = cf->d_params;
        A.pos = centroid ? cf->d_centre : d_pos;
        A.park = cf->d_park;
        A.epart = cf->d_epart;
        A.box = ctx->box;
        if (d_energy) hipLaunchKernelGGL((k_compound<true>), dim3(cf->n_blocks), dim3(AMM_CB_BLOCK), 0, ctx->stream, A, cf->prog.d, cf->d_tab);
        else hipLaunchKernelGGL((k_compound<false>), dim3(cf->n_blocks), dim3(AMM_CB_BLOCK), 0, ctx->stream, A, cf->prog.d, cf->d_tab);
        AMM_HIP(hipGetLastError());
    }
    // (a force without bonds still writes its rows: it may be the first member of its group)
    const dim3 grid(std::max(1, (n + 255) / 256));
    if (centroid)
        hipLaunchKernelGGL(k_compound_spread, grid, dim3(256), 0, ctx->stream, n, cf->d_a_ptr, cf->d_a_grp, cf->d_a_w, cf->d_W, cf->d_ref_ptr,
                           cf->d_rec_src, cf->d_park, d_force, accumulate);
    else
        hipLaunchKernelGGL(k_compound_gather, grid, dim3(256), 0, ctx->stream, n, cf->d_ref_ptr, cf->d_rec_src, cf->d_park, d_force, accumulate);
    AMM_HIP(hipGetLastError());
    if (d_energy && cf->n_bonds > 0) return amm_reduce_add(ctx, cf->d_epart, cf->n_blocks, 1.0, d_energy);
    return 0;
}

// ---- host ----
static int cb_upload_weights(amm_ctx *ctx, CompoundForce *cf, const double *w) {
    std::vector<double> aw(cf->n_members);
    for (int m = 0; m < cf->n_members; ++m) aw[m] = w[cf->a_member[m]];
    AMM_HIP(hipStreamSynchronize(ctx->stream));     // ordered after any kernel already queued on the stream that reads the old values
    AMM_HIP(hipMemcpy(cf->d_g_w, w, sizeof(double) * cf->n_members, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(cf->d_a_w, aw.data(), sizeof(double) * cf->n_members, hipMemcpyHostToDevice));
    return 0;
}

// every group's weights are finite and sum to something other than zero
static int cb_check_weights(const char *who, const int32_t *g_ptr, const double *w, int n_groups) {
    for (int g = 0; g < n_groups; ++g) {
        double W = 0.0;
        for (int m = g_ptr[g]; m < g_ptr[g + 1]; ++m) W += w[m];
        if (!std::isfinite(W) || W == 0.0) {
            amm_set_error(std::string(who) + ": the weights of group " + std::to_string(g) + " sum to " + std::to_string(W) + " (a centre needs a non-zero total weight)");
            return 1;
        }
    }
    return 0;
}

int amm_compound_create_impl(amm_ctx *ctx, int n_slots, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals,
                             int nglobal, const int32_t *var_kinds, const int32_t *var_slots, int n_vars, const int32_t *h_idx,
                             const double *h_params, int n_bonds, int n_params, int periodic, const int32_t *g_ptr, const int32_t *g_atoms,
                             const double *g_weights, int n_groups, CompoundForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_compound_create: " + what);
        return 1;
    };
    const int n = ctx->n;
    if (n_slots < 1 || n_slots > AMM_COMPOUND_MAX_SLOTS)
        return fail(std::to_string(n_slots) + " particles (or groups) per bond (1 .. " + std::to_string(AMM_COMPOUND_MAX_SLOTS) + ")");
    if (n_vars < 0 || n_vars > AMM_COMPOUND_MAX_VARS) return fail(std::to_string(n_vars) + " geometric variables (limit " + std::to_string(AMM_COMPOUND_MAX_VARS) + ")");
    if (n_params < 0 || n_params > AMM_TERM_MAX_PARAMS) return fail(std::to_string(n_params) + " per-bond parameters (limit " + std::to_string(AMM_TERM_MAX_PARAMS) + ")");
    if (n_bonds < 0 || n_groups < 0) return fail("a negative count");
    if (n_params > 0 && n_bonds > 0 && !h_params) return fail("null parameter array");
    if (periodic && !ctx->has_box) return fail("periodic bonds, but the context has no periodic box");
    if (ctx->world > 1) return fail("a compound-bond force (AMM_FORCE_COMPOUND) runs on a single rank");
    if ((long long)n_bonds * std::max(n_vars, 1) * 4 > (long long)INT_MAX) return fail("too many (bond, variable, role) records for a 32-bit index");
    VarTable tab;
    if (var_table_fill("amm_compound_create", var_kinds, var_slots, n_vars, n_slots, AMM_CVAR_X, "the unknown kind ", "",
                       "beyond the bond (" + std::to_string(n_slots) + " slots)", tab, nullptr))
        return 1;
    if (amm_expr_program_validate("amm_compound_create", code, ncode, nconst, nglobal, n_vars, n_params)) return 1;
    const bool centroid = n_groups > 0;
    int n_members = 0;
    if (centroid) {
        if (!g_ptr || !g_atoms || !g_weights) return fail("null group arrays");
        if (g_ptr[0] != 0) return fail("the group offsets do not start at 0");
        for (int g = 0; g < n_groups; ++g)
            if (g_ptr[g + 1] <= g_ptr[g]) return fail("group " + std::to_string(g) + " is empty");
        n_members = g_ptr[n_groups];
        for (int m = 0; m < n_members; ++m)
            if (g_atoms[m] < 0 || g_atoms[m] >= n) return fail("atom index " + std::to_string(g_atoms[m]) + " of a group is out of range");
        if (cb_check_weights("amm_compound_create", g_ptr, g_weights, n_groups)) return 1;
    }
    const int limit = centroid ? n_groups : n;
    for (size_t t = 0; t < (size_t)n_bonds * n_slots; ++t)
        if (h_idx[t] < 0 || h_idx[t] >= limit)
            return fail(std::string(centroid ? "group" : "atom") + " index " + std::to_string(h_idx[t]) + " of bond " + std::to_string(t / n_slots) + " is out of range");
    AMM_HIP(hipSetDevice(ctx->device));
    CompoundForce *cf = new CompoundForce();
    cf->n_slots = n_slots;
    cf->n_vars = n_vars;
    while ((1 << cf->shift) < n_vars) cf->shift++;
    cf->n_bonds = n_bonds;
    cf->n_params = n_params;
    cf->periodic = periodic ? 1 : 0;
    cf->n_groups = n_groups;
    cf->n_members = n_members;
    const int per_block = AMM_CB_BLOCK >> cf->shift;
    cf->n_blocks = std::max(1, (n_bonds + per_block - 1) / per_block);
    cf->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    // CSR of the records per atom (or per group): bond order, then variable, then role
    std::vector<int> ptr, src;
    csr_of_records(limit, [&](auto &&visit) {
        for (int b = 0; b < n_bonds; ++b)
            for (int k = 0; k < n_vars; ++k)
                for (int r = 0; r < cvar_arity(var_kinds[k]); ++r) visit(h_idx[(size_t)b * n_slots + var_slots[4 * k + r]], (b * n_vars + k) * 4 + r);
    }, ptr, src);
    auto alloc = [&]() {
        if (cf->prog.upload(ctx, false)) return 1;
        if (amm_upload(&cf->d_tab, &tab, 1)) return 1;
        if (amm_upload(&cf->d_idx, h_idx, (size_t)n_bonds * n_slots)) return 1;
        if (amm_upload(&cf->d_params, h_params, (size_t)n_bonds * n_params)) return 1;
        if (amm_upload(&cf->d_ref_ptr, ptr.data(), ptr.size())) return 1;
        if (amm_upload(&cf->d_rec_src, src.data(), src.size())) return 1;
        const size_t park = std::max<size_t>((size_t)n_bonds * n_vars * 12, 1);
        AMM_HIP(hipMalloc(&cf->d_park, sizeof(double) * park));
        AMM_HIP(hipMemset(cf->d_park, 0, sizeof(double) * park));
        AMM_HIP(hipMalloc(&cf->d_epart, sizeof(double) * cf->n_blocks));
        if (centroid) {
            // memberships per atom, in group order (and member order within a group)
            std::vector<int> aptr, agrp(n_members), group_of(n_members);
            for (int g = 0; g < n_groups; ++g)
                for (int m = g_ptr[g]; m < g_ptr[g + 1]; ++m) group_of[m] = g;
            csr_of_records(n, [&](auto &&visit) {
                for (int m = 0; m < n_members; ++m) visit(g_atoms[m], m);
            }, aptr, cf->a_member);
            for (int at = 0; at < n_members; ++at) agrp[at] = group_of[cf->a_member[at]];
            if (amm_upload(&cf->d_g_ptr, g_ptr, (size_t)n_groups + 1)) return 1;
            if (amm_upload(&cf->d_g_atom, g_atoms, (size_t)n_members)) return 1;
            if (amm_upload(&cf->d_a_ptr, aptr.data(), aptr.size())) return 1;
            if (amm_upload(&cf->d_a_grp, agrp.data(), agrp.size())) return 1;
            AMM_HIP(hipMalloc(&cf->d_g_w, sizeof(double) * n_members));
            AMM_HIP(hipMalloc(&cf->d_a_w, sizeof(double) * n_members));
            AMM_HIP(hipMalloc(&cf->d_centre, sizeof(double) * 3 * n_groups));
            AMM_HIP(hipMalloc(&cf->d_W, sizeof(double) * n_groups));
            if (cb_upload_weights(ctx, cf, g_weights)) return 1;
        }
        return 0;
    };
    if (alloc()) {
        amm_compound_free(cf);
        return 1;
    }
    *out = cf;
    return 0;
}

int amm_compound_set_globals_impl(amm_ctx *ctx, CompoundForce *cf, const double *globals, int nglobal) {
    return cf->prog.set_globals(ctx, "amm_compound_set_globals", globals, nglobal);
}

int amm_compound_set_params_impl(amm_ctx *ctx, CompoundForce *cf, const double *h_params, int n_bonds, int n_params) {
    const size_t count = (size_t)cf->n_bonds * cf->n_params;
    if (n_bonds != cf->n_bonds || n_params != cf->n_params || (count > 0 && !h_params)) {
        amm_set_error("amm_compound_set_params: the force has " + std::to_string(cf->n_bonds) + " bonds of " + std::to_string(cf->n_params) +
                      " parameters, " + std::to_string(n_bonds) + " x " + std::to_string(n_params) + " given");
        return 1;
    }
    if (!count) return 0;
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    AMM_HIP(hipMemcpy(cf->d_params, h_params, sizeof(double) * count, hipMemcpyHostToDevice));
    return 0;
}

int amm_compound_set_weights_impl(amm_ctx *ctx, CompoundForce *cf, const double *weights, int n_members) {
    if (cf->n_groups == 0) {
        amm_set_error("amm_compound_set_weights: the force has no groups (its bonds join particles)");
        return 1;
    }
    if (n_members != cf->n_members || !weights) {
        amm_set_error("amm_compound_set_weights: the groups have " + std::to_string(cf->n_members) + " members, " + std::to_string(n_members) + " weights given");
        return 1;
    }
    std::vector<int> g_ptr(cf->n_groups + 1);
    AMM_HIP(hipMemcpy(g_ptr.data(), cf->d_g_ptr, sizeof(int) * g_ptr.size(), hipMemcpyDeviceToHost));
    if (cb_check_weights("amm_compound_set_weights", g_ptr.data(), weights, cf->n_groups)) return 1;
    return cb_upload_weights(ctx, cf, weights);
}

void amm_compound_free(CompoundForce *cf) {
    if (!cf) return;
    for (void *p : {(void *)cf->prog.d, (void *)cf->d_tab, (void *)cf->d_idx, (void *)cf->d_params, (void *)cf->d_park, (void *)cf->d_epart,
                    (void *)cf->d_ref_ptr, (void *)cf->d_rec_src, (void *)cf->d_g_ptr, (void *)cf->d_g_atom, (void *)cf->d_g_w, (void *)cf->d_centre,
                    (void *)cf->d_W, (void *)cf->d_a_ptr, (void *)cf->d_a_grp, (void *)cf->d_a_w})
        if (p) (void)hipFree(p);
    delete cf;
}
