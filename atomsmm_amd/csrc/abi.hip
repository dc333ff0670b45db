// atomsmm_amd/csrc/abi.hip -- extern "C" entry points declared in include/atomsmm_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "amm_ctx.h"
#include "cluster.h"
#include "pair_expr_vm.h"

int amm_pair_setup_grid(amm_ctx *ctx, PairForce *pf);
static bool amm_family_allows_cluster(int family, int flags) {
    const bool tab_family = family == AMM_NEAR_NONE || family == AMM_NEAR_SHIFT || family == AMM_NEAR_FSWITCH || family == AMM_DAMPED || family == AMM_NONBONDED;
    return tab_family && !(flags & (AMM_GROUP_LJ | AMM_GROUP_Q));
}
int amm_bonded_arity(int kind);
int amm_bonded_npar(int kind);

static thread_local std::string g_error;
void amm_set_error(const std::string &msg) { g_error = msg; }

template <typename T>
static int upload(T **dst, const T *src, size_t n) {
    AMM_HIP(hipMalloc(dst, sizeof(T) * std::max<size_t>(n, 1)));
    if (n) AMM_HIP(hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}

// exclusion pairs -> symmetric CSR in original atom indices (amm_pair_create)
static int amm_excl_csr(int n, const int32_t *h_excl, int n_excl, std::vector<int> &ptr, std::vector<int> &idx) {
    ptr.assign(n + 1, 0);
    for (int e = 0; e < n_excl; ++e) {
        int i = h_excl[2 * e], j = h_excl[2 * e + 1];
        if (i < 0 || j < 0 || i >= n || j >= n) {
            amm_set_error("amm_pair_create: exclusion index out of range");
            return 1;
        }
        if (i == j) continue;
        ptr[i + 1]++;
        ptr[j + 1]++;
    }
    for (int i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    idx.assign(ptr[n], 0);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int e = 0; e < n_excl; ++e) {
        int i = h_excl[2 * e], j = h_excl[2 * e + 1];
        if (i == j) continue;
        idx[fill[i]++] = j;
        idx[fill[j]++] = i;
    }
    return 0;
}

extern "C" {

int amm_abi_version(void) { return AMM_ABI_VERSION; }
const char *amm_last_error(void) { return g_error.c_str(); }

int amm_create(int32_t n_atoms, const double h_box[3], int32_t device, void *stream, amm_ctx **out) {
    if (!out || n_atoms <= 0) {
        amm_set_error("amm_create: bad arguments");
        return 1;
    }
    for (int k = 0; h_box && k < 3; ++k)
        if (!(h_box[k] > 0.0)) {
            amm_set_error("amm_create: box edges must be positive (orthorhombic periodic box)");
            return 1;
        }
    int ndev = 0;
    AMM_HIP(hipGetDeviceCount(&ndev));
    if (ndev <= 0) {
        amm_set_error("amm_create: no HIP device visible (the HIP path has no CPU fallback)");
        return 1;
    }
    AMM_HIP(hipSetDevice(device));
    amm_ctx *ctx = new amm_ctx();
    ctx->n = n_atoms;
    ctx->device = device;
    ctx->stream = (hipStream_t)stream;
    ctx->has_box = h_box != nullptr;       // (no box: free-space forces and non-periodic terms only; nothing reads ctx->box)
    for (int k = 0; k < 3; ++k) {
        ctx->box.L[k] = h_box ? h_box[k] : 0.0;
        ctx->box.invL[k] = h_box ? 1.0 / h_box[k] : 0.0;
    }
    AMM_HIP(hipMalloc(&ctx->d_scratch, sizeof(double) * ((n_atoms + 255) / 256 + 8)));
    *out = ctx;
    return 0;
}

int amm_destroy(amm_ctx *ctx) {
    if (!ctx) return 0;
    // (with a communicator the wait is bounded and a stuck collective is aborted: comm.hip; then the stream drains)
    amm_comm_destroy_impl(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &f : ctx->forces) amm_family(f.type).free(f.obj);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    if (ctx->d_expr_part) (void)hipFree(ctx->d_expr_part);
    if (ctx->d_fscratch) (void)hipFree(ctx->d_fscratch);
    if (ctx->constraints) amm_constraints_free(ctx->constraints);
    amm_drude_steps_free(ctx);
    for (MinObj *mo : ctx->minimizers) amm_min_free(mo);
    if (ctx->alt_x) (void)hipFree(ctx->alt_x);
    if (ctx->alt_v) (void)hipFree(ctx->alt_v);
    if (ctx->alt_f) (void)hipFree(ctx->alt_f);
    amm_mol_free(ctx);
    amm_vsite_free(ctx);
    delete ctx;
    return 0;
}

int amm_set_stream(amm_ctx *ctx, void *stream) {
    ctx->stream = (hipStream_t)stream;
    return 0;
}

int amm_set_slice(amm_ctx *ctx, int32_t rank, int32_t world) {
    if (world < 1 || rank < 0 || rank >= world) {
        amm_set_error("amm_set_slice: need 0 <= rank < world");
        return 1;
    }
    for (auto &f : ctx->forces) {
        const PairForce *pf = f.pair();
        if (pf && pf->free_space && world > 1) {
            amm_set_error("amm_set_slice: a free-space pair force runs on a single rank");
            return 1;
        }
        if (amm_family(f.type).single_rank && world > 1) {
            amm_set_error(std::string("amm_set_slice: ") + amm_family(f.type).noun + " (" + amm_family(f.type).tag + ") runs on a single rank");
            return 1;
        }
        if (pf && pf->built) {
            amm_set_error("amm_set_slice must be called before the first force evaluation");
            return 1;
        }
    }
    ctx->rank = rank;
    ctx->world = world;
    return 0;
}

int amm_synchronize(amm_ctx *ctx) {
    return amm_comm_wait_impl(ctx, "amm_synchronize");         // (hipStreamSynchronize when the context has no communicator)
}

int amm_check(amm_ctx *ctx) {
    if (amm_comm_wait_impl(ctx, "amm_check")) return 1;
    if (ctx->constraints && amm_constraints_failed(ctx, ctx->constraints)) {
        amm_set_error("constraint solver did not converge (SHAKE / RATTLE, 500 iterations): time step too large or bad geometry");
        return 2;
    }
    if (!ctx->drude_steps.empty()) {
        const int flagged = amm_drude_step_flagged(ctx);
        if (flagged < 0) {
            amm_set_error("amm_check: reading the hard wall flag of the Drude step failed");
            return 1;
        }
        if (flagged) {
            amm_set_error("Drude particle moved too far beyond hard wall constraint");
            return 2;
        }
    }
    for (size_t id = 0; id < ctx->forces.size(); ++id) {
        if (ManyForce *mf = ctx->forces[id].as<ManyForce>()) {
            int need = 0, capacity = 0;
            const int over = amm_many_overflow(mf, &need, &capacity);
            if (over < 0) {
                amm_set_error("amm_check: reading the flag of many-particle force " + std::to_string(id) + " failed");
                return 1;
            }
            if (over) {
                amm_set_error("neighbour table overflow in many-particle force " + std::to_string(id) + " (AMM_FORCE_MANY_PARTICLE): a particle has " +
                              std::to_string(need) + " neighbours > capacity " + std::to_string(capacity) +
                              " (option many_capacity); the energy and the forces of that evaluation are unspecified");
                return 2;
            }
        }
        PairForce *pf = ctx->forces[id].pair();
        if (pf && pf->cl && pf->cl->built) {
            int cf[8];
            AMM_HIP(hipMemcpy(cf, pf->cl->d_flags, sizeof(cf), hipMemcpyDeviceToHost));
            if (cf[7]) {
                amm_set_error("molecule-row list of pair force " + std::to_string(id) + ": a cell holds more molecules than its table (" +
                              std::to_string(pf->cl->capc) + ") or a molecule stretched beyond " + std::to_string(pf->cl->rext) +
                              " nm from its first atom; forces since the last rebuild may be incomplete");
                return 2;
            }
            if (cf[1]) {
                amm_set_error("molecule-row list overflow in pair force " + std::to_string(id) + ": " + std::to_string(cf[2]) +
                              " partners > capacity " + std::to_string(pf->cl->cap) + "; forces since the last rebuild are incomplete");
                return 2;
            }
        }
        if (pf && pf->small && amm_small_group_failed(pf->small) != 0) {
            amm_set_error("interaction-group pair force " + std::to_string(id) + ": a force on an atom of the small set exceeds the range of "
                          "the fixed-point sums (1e6 kJ/mol/nm per wavefront: overlapping atoms, or NaN positions)");
            return 2;
        }
        if (!pf || !pf->built) continue;
        // (a hidden child is reported under its parent's id: the caller never saw the child's)
        const std::string who = pf->hybrid_rest ? std::to_string(pf->profile_id) + " (per-atom part of its hybrid list)" : std::to_string(id);
        int flags[16];
        AMM_HIP(hipMemcpy(flags, pf->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
        if (pf->d_active && flags[8] > pf->active_cap) {
            amm_set_error("interaction-group list of pair force " + who + ": " + std::to_string(flags[8]) +
                          " rows hold entries > the " + std::to_string(pf->active_cap) +
                          " the traversal covers (more than twice the first build's); forces since the last rebuild are incomplete");
            return 2;
        }
        if (flags[7]) {
            amm_set_error("cell list overflow in pair force " + who + ": a cell holds " + std::to_string(flags[6]) +
                          " atoms > capacity " + std::to_string(pf->capc) + " (local density more than doubled since the first build)");
            return 2;
        }
        if (flags[1]) {
            amm_set_error("neighbour list overflow in pair force " + who + ": " + std::to_string(flags[2]) +
                          " neighbours > capacity " + std::to_string(pf->cap) +
                          "; forces since the last rebuild are incomplete");
            return 2;
        }
    }
    return 0;
}

// Verlet buffers and list radii of a pair force from the buffer it asked for and the context's box (amm_pair_create; amm_set_box)
static void pair_derive_buffers(amm_ctx *ctx, PairForce *pf) {
    const amm_pair_desc *desc = &pf->desc;
    double Lmin = std::min(ctx->box.L[0], std::min(ctx->box.L[1], ctx->box.L[2]));
    double skin = std::min(pf->skin_req, std::max(0.0, 0.5 * Lmin - desc->rc) * 0.999);
    pf->skin = skin;
    // a force guarded by step(rc0 - r) (the discount of FarNonbondedForce, forces.py:714; group 31 of RESPASystem) vanishes
    // beyond rc0 whatever its nominal cutoff: its list needs to reach rc0 only
    const double reach = ((desc->flags & AMM_GUARD_RC0) && desc->rc0 > 0.0) ? std::min(desc->rc, desc->rc0) : desc->rc;
    pf->rlist = reach + skin;
    pf->rlist_build = pf->rlist + 2e-4;   // fp32 build: positions carry ~1e-6 nm rounding, superset is harmless
    // outer buffer: large enough that the cell-based build is rare (hydrogens consume 0.05 nm in ~2 outer steps)
    // default: single list (skin_out = skin).  Measured at C3: the prune pass costs about as much as a cell build
    // (both are bound by L1 line-access rate / instruction issue), so the dual list only pays for slow-moving systems.
    double skin_out = pf->skin_out_req > 0 ? pf->skin_out_req : skin;
    skin_out = std::max(skin, std::min(skin_out, std::max(0.0, 0.5 * Lmin - desc->rc) * 0.999));
    pf->skin_out = skin_out;
    pf->rlist_out_build = reach + skin_out + 2e-4;
}

// what sharing a list does to the buffers of guest and host (amm_pair_share_list; amm_set_box after it has derived both again)
static void share_buffers(PairForce *g, PairForce *h) {
    // the guest's skin must be consumed no later than the host's: same displacement trigger
    g->skin = std::min(g->skin, h->skin);
    h->skin = g->skin;
    g->skin_out = h->skin_out;
    h->rlist = h->desc.rc + h->skin;
    h->rlist_build = h->rlist + 2e-4;
    if (h->skin_out < h->skin) h->skin_out = h->skin;
    h->rlist_out_build = h->desc.rc + h->skin_out + 2e-4;
    h->rnear_build = g->rlist_build;
}

// amm_pair_create, and amm_pair_expr_create with the program of its force (`expr`, owned by the force from here on)
static int pair_create_common(amm_ctx *ctx, const amm_pair_desc *desc, const double *h_q, const double *h_sigma,
                              const double *h_eps, const int32_t *h_excl, int32_t n_excl, double skin, int32_t *force_id, PairExpr *expr) {
    const bool free_space = (desc->flags & AMM_FREE_SPACE) != 0;
    if (!free_space && !ctx->has_box) {
        amm_set_error("amm_pair_create: the context has no periodic box (only AMM_FREE_SPACE pair forces run without one)");
        return 1;
    }
    if (!free_space && !(desc->rc > 0.0)) {
        amm_set_error("amm_pair_create: cutoff must be positive");
        return 1;
    }
    if (free_space) {
        std::string why;
        if (!amm_free_supported(*desc, why)) {
            amm_set_error("amm_pair_create (AMM_FREE_SPACE): " + why);
            return 1;
        }
        if (ctx->n > AMM_FREE_MAX_ATOMS) {
            amm_set_error("amm_pair_create: a free-space pair force walks all n^2 pairs and takes at most " + std::to_string(AMM_FREE_MAX_ATOMS) +
                          " atoms (this context has " + std::to_string(ctx->n) + ")");
            return 1;
        }
        if (ctx->world > 1) {
            amm_set_error("amm_pair_create: a free-space pair force runs on a single rank");
            return 1;
        }
    }
    PairForce *pf = new PairForce();
    pf->desc = *desc;
    pf->n = ctx->n;
    pf->skin_out_req = ctx->skin_out;
    pf->free_space = free_space;
    if (ctx->n >= (1 << 26)) {      // the traversal addresses the sorted copies with 32-bit byte offsets (32 B per slot)
        amm_set_error("amm_pair_create: more than 2^26 atoms are not supported");
        amm_pair_free(pf);
        return 1;
    }
    if (amm_pair_build_consts(*desc, pf->pc) || (!free_space && amm_pair_build_table(pf))) {
        amm_pair_free(pf);
        return 1;
    }
    const int n = ctx->n;
    if (free_space) {
        // no radial table, no grid, no list: the exclusion CSR and the parameters in atom order are all such a force keeps
        std::memset(&pf->pc.tab, 0, sizeof(pf->pc.tab));
        pf->pc.tab.ss_first = -1;
        pf->last_kind = 4;
        std::memset(&pf->grid, 0, sizeof(pf->grid));
        std::vector<int> ptr, idx;
        if (amm_excl_csr(n, h_excl, n_excl, ptr, idx)) {
            amm_pair_free(pf);
            return 1;
        }
        // (the kernel reads the charges and one (sigma/2, 2 sqrt(eps)) record per atom: no separate sigma / epsilon arrays)
        if (upload(&pf->d_excl_ptr, ptr.data(), ptr.size()) || upload(&pf->d_excl_idx, idx.data(), idx.size()) ||
            hipMalloc(&pf->d_q, sizeof(double) * n) != hipSuccess || hipMalloc(&pf->d_lj_s, sizeof(double2) * n) != hipSuccess) {
            amm_set_error("amm_pair_create: device allocation failed");
            amm_pair_free(pf);
            return 1;
        }
        *force_id = pf->id = amm_force_register(ctx, AMM_FORCE_PAIR, pf);
        return amm_pair_set_params(ctx, *force_id, h_q, h_sigma, h_eps);
    }
    // default Verlet buffer: 0.1 nm on one GPU (C3: list build 0.58 x 320 us per step against +30 % pair work at 0.2 nm);
    // a rank's slice makes the pair kernels 2 - 5 x cheaper but the rebuild only 1.6 - 2 x (scripts/probe_pair.py --world N),
    // so the optimum moves to a larger buffer: 0.15 nm for 2 ranks, 0.2 nm beyond
    if (skin < 0) skin = ctx->world >= 4 ? 0.2 : (ctx->world >= 2 ? 0.15 : 0.1);
    pf->skin_req = skin;
    pair_derive_buffers(ctx, pf);
    if (amm_pair_setup_grid(ctx, pf)) {
        amm_pair_free(pf);
        return 1;
    }
    // exclusions -> symmetric CSR in original atom indices
    std::vector<int> ptr, idx;
    if (amm_excl_csr(n, h_excl, n_excl, ptr, idx)) {
        amm_pair_free(pf);
        return 1;
    }
    if (upload(&pf->d_excl_ptr, ptr.data(), ptr.size()) || upload(&pf->d_excl_idx, idx.data(), idx.size())) {
        amm_pair_free(pf);
        return 1;
    }
    if (desc->family == AMM_SOFTCORE || (desc->flags & (AMM_GROUP_LJ | AMM_GROUP_Q))) {
        pf->h_excl_ptr = ptr;
        pf->h_excl_idx = idx;
    }
    // Three-site molecules take molecule rows on the force-only hot path (cluster.h).  A box of nothing else: molecule rows only.
    // Molecules next to other atoms (ions, a solute, a chain; at least half of the atoms in molecules): a hybrid list -- molecule
    // rows for the pairs of two molecules, per-atom rows kept by a hidden child force for every pair with an atom outside them.
    // The reference makes no such distinction (forces.py:299-312 copies any particle list, every exception -> exclusion).
    std::vector<int> rest_atoms;
    if (amm_family_allows_cluster(desc->family, desc->flags) && !ctx->creating_rest) {
        std::vector<int> mol_first;
        amm_cluster_classify(n, ptr, idx, mol_first, rest_atoms);
        pf->n_mol = (int)mol_first.size();
        pf->n_rest = (int)rest_atoms.size();
        if (pf->n_mol > 0 && pf->n_rest == 0) {
            pf->cluster_ok = true;
        } else if (pf->n_mol > 0 && 2 * 3 * (long)pf->n_mol >= (long)n) {
            pf->cluster_ok = pf->hybrid = true;
            pf->h_mol_first = mol_first;
            if (upload(&pf->d_mol_first, mol_first.data(), mol_first.size()) || upload(&pf->d_rest_idx, rest_atoms.data(), rest_atoms.size())) return 1;
        }
    }
    AMM_HIP(hipMalloc(&pf->d_q, sizeof(double) * n));
    AMM_HIP(hipMalloc(&pf->d_hsig, sizeof(double) * n));
    AMM_HIP(hipMalloc(&pf->d_seps2, sizeof(double) * n));
    const int nc = pf->grid.ncell;
    pf->ncell_alloc = nc;
    AMM_HIP(hipMalloc(&pf->d_cell_of, sizeof(int) * n));
    AMM_HIP(hipMalloc(&pf->d_cell_count, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMemset(pf->d_cell_count, 0, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMalloc(&pf->d_cell_start, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMalloc(&pf->d_cell_count_lj, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMemset(pf->d_cell_count_lj, 0, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMalloc(&pf->d_cell_start_lj, sizeof(int) * (nc + 1)));
    AMM_HIP(hipMalloc(&pf->d_cls, sizeof(int) * n));
    AMM_HIP(hipMalloc(&pf->d_perm, sizeof(int) * n));
    AMM_HIP(hipMalloc(&pf->d_inv_perm, sizeof(int) * n));
    AMM_HIP(hipMalloc(&pf->d_posq_s, sizeof(double4) * n));
    AMM_HIP(hipMalloc(&pf->d_lj_s, sizeof(double2) * n));
    AMM_HIP(hipMalloc(&pf->d_pos4f_s, sizeof(float4) * n));
    AMM_HIP(hipMalloc(&pf->d_xref, sizeof(double) * 3 * n));
    AMM_HIP(hipMalloc(&pf->d_xref_out, sizeof(double) * 3 * n));
    AMM_HIP(hipMalloc(&pf->d_flags, sizeof(int) * 16));
    AMM_HIP(hipMemset(pf->d_flags, 0, sizeof(int) * 16));
    AMM_HIP(hipMalloc(&pf->d_ticket, sizeof(int) * 4 * AMM_TICKET_INTS));
    AMM_HIP(hipMemset(pf->d_ticket, 0, sizeof(int) * 4 * AMM_TICKET_INTS));
    AMM_HIP(hipMalloc(&pf->d_counters, sizeof(unsigned long long) * 8));
    AMM_HIP(hipMemset(pf->d_counters, 0, sizeof(unsigned long long) * 8));
    pf->expr = expr;          // (the force owns the program once it is registered: amm_pair_free)
    *force_id = pf->id = amm_force_register(ctx, AMM_FORCE_PAIR, pf);
    if (amm_pair_set_params(ctx, *force_id, h_q, h_sigma, h_eps)) return 1;
    if (pf->hybrid) {
        // the child: same particles, parameters, exclusions and Verlet buffer; its list keeps the pairs with a rest atom (code 2)
        int32_t child_id = -1;
        ctx->creating_rest = true;
        // (twice the Verlet buffer of the molecule rows: walking the per-atom part costs a tenth of walking the molecule rows, rebuilding
        // it half as much as rebuilding them -- at config C5 its optimum lies at a larger buffer; the two lists are independent)
        const int rc = amm_pair_create(ctx, desc, h_q, h_sigma, h_eps, h_excl, n_excl, pf->skin * ctx->opt_rest_skin_factor, &child_id);
        ctx->creating_rest = false;
        if (rc) return 1;
        PairForce *child = ctx->forces[child_id].pair();
        child->hybrid_rest = true;
        child->profile_id = pf->id;
        std::vector<float> code(n, 1.0f);
        for (int i : rest_atoms) code[i] = 2.0f;
        if (upload(&child->d_member, code.data(), code.size())) return 1;
        pf->rest = child;
    }
    return 0;
}

int amm_pair_create(amm_ctx *ctx, const amm_pair_desc *desc, const double *h_q, const double *h_sigma,
                    const double *h_eps, const int32_t *h_excl, int32_t n_excl, double skin, int32_t *force_id) {
    if (!ctx || !desc || !h_q || !h_sigma || !h_eps || !force_id) {
        amm_set_error("amm_pair_create: null argument");
        return 1;
    }
    if (desc->family == AMM_PAIR_EXPR) {
        amm_set_error("amm_pair_create: a pair-expression force (AMM_PAIR_EXPR) comes with its program: amm_pair_expr_create");
        return 1;
    }
    if (desc->family < AMM_NEAR_NONE || desc->family > AMM_LJ_VIRIAL) {
        amm_set_error("amm_pair_create: unknown family");
        return 1;
    }
    return pair_create_common(ctx, desc, h_q, h_sigma, h_eps, h_excl, n_excl, skin, force_id, nullptr);
}

// CustomNonbondedForce(any energy text): the compiled text (atomsmm_amd/expr.py: compile_pair) and the raw per-particle parameters
int amm_pair_expr_create(amm_ctx *ctx, const amm_pair_desc *desc, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst,
                         const double *globals, int32_t nglobal, const double *h_p0, const double *h_p1, const double *h_p2,
                         const int32_t *h_excl, int32_t n_excl, double skin, int32_t *force_id) {
    if (!ctx || !desc || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals)) {
        amm_set_error("amm_pair_expr_create: null argument");
        return 1;
    }
    if (desc->family != AMM_PAIR_EXPR) {
        amm_set_error("amm_pair_expr_create: the descriptor's family must be AMM_PAIR_EXPR");
        return 1;
    }
    if (desc->flags & AMM_FREE_SPACE) {
        amm_set_error("amm_pair_expr_create: a pair-expression force (AMM_PAIR_EXPR) walks neighbour rows in a periodic box: no AMM_FREE_SPACE");
        return 1;
    }
    if ((desc->flags & AMM_SWITCH) && !(desc->rswitch >= 0.0 && desc->rswitch < desc->rc)) {
        amm_set_error("amm_pair_expr_create: the switch needs 0 <= rswitch < rc");
        return 1;
    }
    if (amm_pair_expr_validate(code, ncode, nconst, nglobal)) return 1;
    // only rc, rswitch, the switch flag and the sign are read: the other fields do not reach the constants
    amm_pair_desc d;
    std::memset(&d, 0, sizeof(d));
    d.family = AMM_PAIR_EXPR;
    d.flags = desc->flags & AMM_SWITCH;
    d.degree = 1;
    d.sign = desc->sign;
    d.rc = desc->rc;
    d.rswitch = (desc->flags & AMM_SWITCH) ? desc->rswitch : 0.0;
    PairExpr *px = new PairExpr();
    px->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    amm_pair_expr_scan_tables(px);
    if (px->prog.upload(ctx, false)) {
        amm_pair_expr_free(px);
        return 1;
    }
    const std::vector<double> zero(ctx->n, 0.0);          // (a NULL parameter array: all zero)
    const size_t before = ctx->forces.size();
    const int rc = pair_create_common(ctx, &d, h_p0 ? h_p0 : zero.data(), h_p1 ? h_p1 : zero.data(), h_p2 ? h_p2 : zero.data(), h_excl, n_excl,
                                      skin, force_id, px);
    if (rc && ctx->forces.size() == before) amm_pair_expr_free(px);     // (not registered: nobody else frees the program)
    return rc;
}

int amm_pair_expr_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    if (!pf->expr) {
        amm_set_error("amm_pair_expr_set_globals: not a pair-expression force (AMM_PAIR_EXPR)");
        return 1;
    }
    return pf->expr->prog.set_globals(ctx, "amm_pair_expr_set_globals", globals, nglobal);
}

int amm_pair_expr_set_tables(amm_ctx *ctx, int32_t force_id, int32_t n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                             const int32_t *offsets, const double *data, int32_t n_data) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    if (!pf->expr) {
        amm_set_error("amm_pair_expr_set_tables: not a pair-expression force (AMM_PAIR_EXPR)");
        return 1;
    }
    return amm_pair_expr_tables(ctx, pf->expr, n_tables, kinds, dims, ranges, offsets, data, n_data);
}

int amm_pair_set_lambda(amm_ctx *ctx, int32_t force_id, double value) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    if (pf->expr) {
        amm_set_error("amm_pair_set_lambda: not for a pair-expression force (AMM_PAIR_EXPR): its globals go through amm_pair_expr_set_globals");
        return 1;
    }
    if (pf->free_space) {
        amm_set_error("amm_pair_set_lambda: not for a free-space pair force (AMM_FREE_SPACE)");
        return 1;
    }
    if (pf->desc.family != AMM_SOFTCORE) {
        amm_set_error("amm_pair_set_lambda: not a softcore pair force");
        return 1;
    }
    pf->desc.alpha = value;
    pf->d_lambda_dev = nullptr;        // (a number from the host replaces a device-resident lambda)
    return amm_pair_build_consts(pf->desc, pf->pc);
}

int amm_pair_set_lambda_dev(amm_ctx *ctx, int32_t force_id, const double *d_lambda) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    if (pf->expr) {
        amm_set_error("amm_pair_set_lambda_dev: not for a pair-expression force (AMM_PAIR_EXPR)");
        return 1;
    }
    if (pf->free_space) {
        amm_set_error("amm_pair_set_lambda_dev: not for a free-space pair force (AMM_FREE_SPACE)");
        return 1;
    }
    if (pf->desc.family != AMM_SOFTCORE) {
        amm_set_error("amm_pair_set_lambda_dev: not a softcore pair force");
        return 1;
    }
    if (d_lambda && !(pf->small && ctx->opt_small_group && amm_small_group_supported(pf))) {
        amm_set_error("amm_pair_set_lambda_dev: only the list-free evaluation of a softcore force with a small set reads lambda from the device");
        return 1;
    }
    pf->d_lambda_dev = d_lambda;
    return 0;
}

int amm_pair_set_scale(amm_ctx *ctx, int32_t force_id, double scale) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    pf->desc.sign = scale;
    pf->pc.sign = scale;
    // the pairings cached for the one-pass evaluations depend on the sign (host sign == 1): decide them again
    pf->dual_ok = pf->fuse_ok = -1;
    for (auto &fo : ctx->forces)
        if (fo.type == AMM_FORCE_PAIR && fo.pair()->host == pf) fo.pair()->dual_ok = fo.pair()->fuse_ok = -1;
    // (a hybrid list's per-atom part is a force of its own with its own constants: same scale)
    if (pf->rest) return amm_pair_set_scale(ctx, pf->rest->id, scale);
    return 0;
}

int amm_pair_energy_derivative(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_out) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf || !d_pos || !d_out) return 1;
    if (pf->expr) {
        amm_set_error("amm_pair_energy_derivative: not for a pair-expression force (AMM_PAIR_EXPR): the interpreter differentiates in r only");
        return 1;
    }
    if (pf->free_space) {
        amm_set_error("amm_pair_energy_derivative: not for a free-space pair force (AMM_FREE_SPACE)");
        return 1;
    }
    if (pf->desc.family != AMM_SOFTCORE) {
        amm_set_error("amm_pair_energy_derivative: only the softcore family depends on a global parameter");
        return 1;
    }
    if (!ctx->d_fscratch) AMM_HIP(hipMalloc(&ctx->d_fscratch, sizeof(double) * 3 * (size_t)ctx->n));
    if (!(ctx->opt_positions_private && d_pos == ctx->d_x)) ctx->pos_epoch++;     // (the bound buffer under the caller's promise: unchanged)
    pf->pc.flags |= AMM_DERIV_LAMBDA;
    int rc = -1;
    // (a list-free group force: only the atoms near its small set when a neighbour list vouches for them -- the rows are scratch)
    if (pf->small && ctx->opt_small_group && !pf->built) rc = amm_small_group_eval_impl(ctx, pf, d_pos, ctx->d_fscratch, 0, d_out, nullptr, nullptr, 1);
    if (rc < 0) rc = amm_pair_eval_impl(ctx, pf, d_pos, ctx->d_fscratch, 0, d_out);
    pf->pc.flags &= ~AMM_DERIV_LAMBDA;
    return rc;
}

int amm_pair_energy_states(amm_ctx *ctx, int32_t force_id, const double *d_pos, const double *d_lambdas, int32_t n_states, double *d_out) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    if (pf->expr) {
        amm_set_error("amm_pair_energy_states: not for a pair-expression force (AMM_PAIR_EXPR)");
        return 1;
    }
    if (pf->free_space) {
        amm_set_error("amm_pair_energy_states: not for a free-space pair force (AMM_FREE_SPACE)");
        return 1;
    }
    if (n_states < 1 || n_states > AMM_MAX_STATES) {
        amm_set_error("amm_pair_energy_states: need 1 <= n_states <= AMM_MAX_STATES (" + std::to_string(AMM_MAX_STATES) + ")");
        return 1;
    }
    if (!d_pos || !d_lambdas || !d_out) {
        amm_set_error("amm_pair_energy_states: null argument");
        return 1;
    }
    if (pf->desc.family != AMM_SOFTCORE) {
        amm_set_error("amm_pair_energy_states: only the softcore family depends on a global parameter");
        return 1;
    }
    if (!(ctx->opt_positions_private && d_pos == ctx->d_x)) ctx->pos_epoch++;     // (as amm_pair_energy_derivative)
    if (pf->small && ctx->opt_small_group && !pf->built && amm_small_group_supported(pf))
        return amm_small_group_energy_states(ctx, pf, d_pos, d_lambdas, n_states, d_out);
    // a force on the list path (both sets large): one energy evaluation per lambda, with lambda swapped into the launch constants and
    // restored as amm_pair_energy_derivative does with its flag (the list path never reads a device lambda)
    std::vector<double> lam(n_states);
    AMM_HIP(hipMemcpyAsync(lam.data(), d_lambdas, sizeof(double) * n_states, hipMemcpyDeviceToHost, ctx->stream));
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->d_fscratch) AMM_HIP(hipMalloc(&ctx->d_fscratch, sizeof(double) * 3 * (size_t)ctx->n));
    const double alpha = pf->pc.alpha;
    int rc = 0;
    for (int k = 0; k < n_states && rc == 0; ++k) {
        pf->pc.alpha = lam[k];
        rc = amm_pair_eval_impl(ctx, pf, d_pos, ctx->d_fscratch, 0, d_out + k);
    }
    pf->pc.alpha = alpha;
    return rc;
}

static int share_list_pf(amm_ctx *ctx, PairForce *g, PairForce *h) {
    if (g == h || h->host || g->host || g->rnear_build > 0) {
        amm_set_error("amm_pair_share_list: invalid host/guest combination");
        return 1;
    }
    if ((g->d_member || h->d_member) && !(g->hybrid_rest && h->hybrid_rest)) {
        amm_set_error("amm_pair_share_list: an interaction-group force keeps its own (filtered) neighbour list");
        return 1;
    }
    if (g->built || h->built) {
        amm_set_error("amm_pair_share_list must be called before the first force evaluation");
        return 1;
    }
    if (g->rlist_build > h->rlist_build) {
        amm_set_error("amm_pair_share_list: the guest's list radius exceeds the host's");
        return 1;
    }
    if (h->rnear_build > 0 && h->rnear_build != g->rlist_build) {
        amm_set_error("amm_pair_share_list: the host already serves a guest with a different list radius");
        return 1;
    }
    // identical exclusion sets are required: compare the CSR arrays
    const int n = ctx->n;
    std::vector<int> pa(n + 1), pb(n + 1);
    AMM_HIP(hipMemcpy(pa.data(), g->d_excl_ptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    AMM_HIP(hipMemcpy(pb.data(), h->d_excl_ptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    bool same = pa == pb;
    if (same && pa[n] > 0) {
        std::vector<int> ia(pa[n]), ib(pa[n]);
        AMM_HIP(hipMemcpy(ia.data(), g->d_excl_idx, sizeof(int) * pa[n], hipMemcpyDeviceToHost));
        AMM_HIP(hipMemcpy(ib.data(), h->d_excl_idx, sizeof(int) * pa[n], hipMemcpyDeviceToHost));
        for (int i = 0; i < n && same; ++i) {
            std::sort(ia.begin() + pa[i], ia.begin() + pa[i + 1]);
            std::sort(ib.begin() + pa[i], ib.begin() + pa[i + 1]);
        }
        same = ia == ib;
    }
    if (!same) {
        amm_set_error("amm_pair_share_list: exclusion lists differ");
        return 1;
    }
    share_buffers(g, h);
    g->host = h;
    // both hybrid (same exclusions: the same molecules): the per-atom parts share a list the same way
    if (g->rest && h->rest) return share_list_pf(ctx, g->rest, h->rest);
    return 0;
}

int amm_pair_share_list(amm_ctx *ctx, int32_t force_id, int32_t host_id) {
    PairForce *g = amm_force_get<PairForce>(ctx, force_id), *h = amm_force_get<PairForce>(ctx, host_id);
    if (!g || !h) return 1;
    if (g->hybrid_rest || h->hybrid_rest) {
        amm_set_error("amm_pair_share_list: not a force of the caller's");
        return 1;
    }
    if (g->expr || h->expr) {
        amm_set_error("amm_pair_share_list: a pair-expression force (AMM_PAIR_EXPR) keeps a neighbour list of its own");
        return 1;
    }
    if (g->free_space || h->free_space) {
        amm_set_error("amm_pair_share_list: a free-space pair force (AMM_FREE_SPACE) has no neighbour list to share");
        return 1;
    }
    return share_list_pf(ctx, g, h);
}

int amm_pair_set_params(amm_ctx *ctx, int32_t force_id, const double *h_q, const double *h_sigma, const double *h_eps) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    const int n = pf->n;
    if (pf->expr) {
        // a pair-expression force: its program takes the three slots as the text's own per-particle parameters -- RAW values (any
        // sign), a NULL array = all zero.  Every atom counts as a site (no row is cut short), no charge-less or one-class shortcut.
        const std::vector<double> zero(n, 0.0);
        AMM_HIP(hipStreamSynchronize(ctx->stream));
        AMM_HIP(hipMemcpy(pf->d_q, h_q ? h_q : zero.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        AMM_HIP(hipMemcpy(pf->d_hsig, h_sigma ? h_sigma : zero.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        AMM_HIP(hipMemcpy(pf->d_seps2, h_eps ? h_eps : zero.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        if (pf->h_cls.empty()) {
            pf->h_cls.assign(n, 0);
            AMM_HIP(hipMemcpy(pf->d_cls, pf->h_cls.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        }
        pf->a_sorted_for = nullptr;
        return 0;
    }
    std::vector<double> hs(n), se(n);
    for (int i = 0; i < n; ++i) {
        if (h_eps[i] < 0.0) {
            amm_set_error("amm_pair_set_params: negative epsilon");
            return 1;
        }
        hs[i] = 0.5 * h_sigma[i];          // sigma = 0.5*(sigma1+sigma2)       forces.py:256
        se[i] = 2.0 * std::sqrt(h_eps[i]); // 4*epsilon = 4*sqrt(eps1*eps2)     forces.py:257
    }
    pf->all_q_zero = true;
    for (int i = 0; i < n && pf->all_q_zero; ++i) pf->all_q_zero = h_q[i] == 0.0;
    // ordered after any kernels already queued on the stream
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    AMM_HIP(hipMemcpy(pf->d_q, h_q, sizeof(double) * n, hipMemcpyHostToDevice));
    if (pf->free_space) {
        // the tiles of free.hip read (sigma/2, 2 sqrt(eps)) as one 16-byte record per atom, in atom order; nothing else is kept
        std::vector<double> lj(2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            lj[2 * i] = hs[i];
            lj[2 * i + 1] = se[i];
        }
        AMM_HIP(hipMemcpy(pf->d_lj_s, lj.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice));
        return 0;
    }
    AMM_HIP(hipMemcpy(pf->d_hsig, hs.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(pf->d_seps2, se.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    // interaction-group forces carry the set code of every atom (0 none, 1, 2) in place of a parameter: q for SOFTCORE and
    // AMM_GROUP_LJ (product 2 = a (set 1, set 2) pair), sigma for AMM_GROUP_Q (sigma/2 holds the code).  The neighbour list
    // of such a force keeps only the pairs with code_i * code_j == 2: every other entry would be evaluated to an exact zero.
    {
        const bool by_q = pf->desc.family == AMM_SOFTCORE || (pf->desc.flags & AMM_GROUP_LJ);
        const bool by_sigma = (pf->desc.flags & AMM_GROUP_Q) != 0;
        if (by_q || by_sigma) {
            std::vector<float> member(n);
            for (int i = 0; i < n; ++i) member[i] = (float)(by_q ? h_q[i] : 0.5 * h_sigma[i]);
            if (!pf->d_member) AMM_HIP(hipMalloc(&pf->d_member, sizeof(float) * n));
            AMM_HIP(hipMemcpy(pf->d_member, member.data(), sizeof(float) * n, hipMemcpyHostToDevice));
            // a small set (a solute): no neighbour list at all (group.hip); decided again whenever the codes change
            if (!pf->built && amm_small_group_setup(ctx, pf, member)) return 1;
        }
    }
    // one Lennard-Jones site class?  (water: the oxygens) -- the molecule-row kernels then need no per-atom LJ records
    {
        // (hybrid lists: the molecule rows hold the molecules' atoms only -- the sites that matter are theirs)
        std::vector<char> in_mol;
        if (pf->hybrid) {
            in_mol.assign(n, 0);
            for (int i0 : pf->h_mol_first) in_mol[i0] = in_mol[i0 + 1] = in_mol[i0 + 2] = 1;
        }
        auto skip = [&](int i) { return h_eps[i] == 0.0 || (pf->hybrid && !in_mol[i]); };
        pf->one_site_class = true;
        bool seen = false;
        for (int i = 0; i < n; ++i) {
            if (skip(i)) continue;
            if (!seen) {
                seen = true;
                pf->site_hsig = hs[i];
                pf->site_seps2 = se[i];
            } else if (hs[i] != pf->site_hsig || se[i] != pf->site_seps2) {
                pf->one_site_class = false;
                break;
            }
        }
        if (!seen) pf->site_hsig = pf->site_seps2 = 0.0;
        // ... and one charge?  Then the pairs of two sites have ONE radial force function and a table of their own (pair_tab.h)
        pf->site_one_charge = pf->one_site_class && seen;
        pf->site_q = 0.0;
        bool first = true;
        for (int i = 0; i < n && pf->site_one_charge; ++i) {
            if (skip(i)) continue;
            if (first) {
                first = false;
                pf->site_q = h_q[i];
            } else if (h_q[i] != pf->site_q) {
                pf->site_one_charge = false;
            }
        }
        pf->site_atoms = 0;
        if (pf->hybrid) {
            for (int i0 : pf->h_mol_first)
                for (int a = 0; a < 3; ++a)
                    if (h_eps[i0 + a] != 0.0) pf->site_atoms |= 1 << a;
        } else {
            for (int i = 0; i < n; ++i)
                if (h_eps[i] != 0.0) pf->site_atoms |= 1 << (i % 3);
        }
        const double now[3] = {pf->site_hsig, pf->site_seps2, (pf->one_site_class && pf->site_one_charge) ? pf->site_q : 0.0};
        if (pf->cluster_ok && (now[0] != pf->ss_built_for[0] || now[1] != pf->ss_built_for[1] || now[2] != pf->ss_built_for[2])) {
            AMM_HIP(hipStreamSynchronize(ctx->stream));       // (kernels in flight read the tables about to be replaced)
            if (amm_pair_build_table(pf)) return 1;
            pf->dual_ok = -1;
            pf->fuse_ok = -1;
        }
    }
    // class of each atom for the traversal order: 1 = no Lennard-Jones site (its rows skip the LJ arithmetic)
    std::vector<int> cls(n);
    for (int i = 0; i < n; ++i) cls[i] = h_eps[i] == 0.0 ? 1 : 0;
    AMM_HIP(hipMemcpy(pf->d_cls, cls.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    if (cls != pf->h_cls) {
        // another set of atoms has a site (an epsilon offset crossed zero): the list's order within the cells and the rows' site
        // counts were made for the old one -- rebuild at the next evaluation; guests re-check that their sites are the owner's
        if (!pf->h_cls.empty() && pf->built) pf->force_rebuild = true;
        if (!pf->h_cls.empty() && pf->cl) pf->force_rebuild_c = true;
        pf->h_cls = cls;
        pf->sites_match = -1;
        for (auto &fo : ctx->forces)
            if (fo.type == AMM_FORCE_PAIR && fo.pair()->host == pf) fo.pair()->sites_match = -1;
    }
    // the sorted copies of the parameters that a launch wrote ahead of time (epilogues: pair.hip, cluster.hip) were made with the old
    // ones: no later evaluation may take them for current, whichever force of the list (this one or a guest) they belong to
    {
        PairForce *L = pf->host ? pf->host : pf;
        L->a_sorted_for = nullptr;
        if (L->cl) L->cl->sorted_for = nullptr;
    }
    // dual evaluation needs bitwise equal parameters on guest and host: re-check after any change
    pf->dual_ok = pf->fuse_ok = -1;
    for (auto &fo : ctx->forces)
        if (fo.type == AMM_FORCE_PAIR && fo.pair()->host == pf) fo.pair()->dual_ok = fo.pair()->fuse_ok = -1;
    if (pf->rest) return amm_pair_set_params(ctx, pf->rest->id, h_q, h_sigma, h_eps);
    return 0;
}

int amm_bonded_create(amm_ctx *ctx, int32_t *force_id) {
    BondedSet *bs = new BondedSet();
    std::memset(&bs->near_pc, 0, sizeof(bs->near_pc));
    *force_id = amm_force_register(ctx, AMM_FORCE_BONDED, bs);
    return 0;
}

int amm_bonded_add_terms(amm_ctx *ctx, int32_t force_id, int32_t kind, const int32_t *h_idx, const double *h_params,
                         int32_t n_terms, int32_t periodic, const amm_pair_desc *desc) {
    BondedSet *bs = amm_force_get<BondedSet>(ctx, force_id);
    if (!bs) return 1;
    if (bs->finalized) {
        amm_set_error("amm_bonded_add_terms after finalize");
        return 1;
    }
    if (kind < 0 || kind > 7) {
        amm_set_error("amm_bonded_add_terms: unknown kind");
        return 1;
    }
    if ((periodic || kind == AMM_BOND_EWALD_EXCL) && !ctx->has_box) {
        amm_set_error("amm_bonded_add_terms: periodic terms, but the context has no periodic box");
        return 1;
    }
    if (!bs->h_idx[kind].empty() && bs->periodic[kind] != periodic) {
        amm_set_error("amm_bonded_add_terms: mixed periodic flags within one kind");
        return 1;
    }
    const int ar = amm_bonded_arity(kind), np = amm_bonded_npar(kind);
    if (kind == AMM_BOND_NEAR) {
        if (!desc) {
            amm_set_error("AMM_BOND_NEAR needs a pair descriptor");
            return 1;
        }
        if (bs->has_near && std::memcmp(&bs->near_desc, desc, sizeof(*desc)) != 0) {
            amm_set_error("one bonded set supports a single near-exception descriptor");
            return 1;
        }
        bs->has_near = true;
        bs->near_desc = *desc;
        if (amm_pair_build_consts(*desc, bs->near_pc)) return 1;
    }
    double scale = 1.0;
    if (kind == AMM_BOND_EWALD_EXCL) {
        if (!desc) {
            amm_set_error("AMM_BOND_EWALD_EXCL needs a descriptor carrying alpha and Kc");
            return 1;
        }
        bs->ewald_alpha = desc->alpha;
        bs->ewald_Kc = desc->Kc;
        scale = desc->Kc;
    }
    if (kind == AMM_BOND_LJC && desc) bs->ljc_Kc = desc->Kc;
    bs->periodic[kind] = periodic;
    // Terms whose energy is identically zero are not stored: the exceptions of a water model (chargeprod = 0,
    // epsilon = 0: SURVEY.md 8a-6, `tests/test_systems.py:146` expects their energy to be 0.0) would otherwise be
    // evaluated in every inner RESPA iteration -- 3 of the 6 terms of a flexible water.
    for (int t = 0; t < n_terms; ++t) {
        const double *pr = h_params + (size_t)t * np;
        bool zero = false;
        if (kind == AMM_BOND_LJC || kind == AMM_BOND_NEAR) zero = pr[0] == 0.0 && pr[2] == 0.0;
        else if (kind == AMM_BOND_EWALD_EXCL) zero = pr[0] == 0.0;
        if (zero) continue;
        bs->h_idx[kind].insert(bs->h_idx[kind].end(), h_idx + (size_t)t * ar, h_idx + (size_t)(t + 1) * ar);
        for (int k = 0; k < np; ++k) bs->h_par[kind].push_back(pr[k] * scale);
    }
    return 0;
}

int amm_bonded_finalize(amm_ctx *ctx, int32_t force_id) {
    BondedSet *bs = amm_force_get<BondedSet>(ctx, force_id);
    if (!bs) return 1;
    return amm_bonded_finalize_impl(ctx, bs);
}

int amm_bonded_set_sliced(amm_ctx *ctx, int32_t force_id, int32_t on) {
    BondedSet *bs = amm_force_get<BondedSet>(ctx, force_id);
    if (!bs) return 1;
    bs->sliced = on != 0;
    return 0;
}

int amm_bonded_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_BONDED, nullptr); }

// which layouts amm_bonded_finalize built and which launches they admit (read-only; see include/atomsmm_hip.h)
int amm_bonded_stats(amm_ctx *ctx, int32_t force_id, int64_t *out) {
    BondedSet *bs = amm_force_get<BondedSet>(ctx, force_id);
    if (!bs) return 1;
    if (!out) {
        amm_set_error("amm_bonded_stats: null argument");
        return 1;
    }
    if (!bs->finalized) {
        amm_set_error("amm_bonded_stats before amm_bonded_finalize");
        return 1;
    }
    out[0] = bs->ncomp;
    out[1] = bs->max_comp;
    out[2] = bs->terms_ok ? 1 : 0;
    out[3] = bs->G;                              // lanes per component: the term tables' stride and the inner-components launch's
    out[4] = bs->mol3_ok ? 1 : 0;
    out[5] = bs->mixed_ok ? 1 : 0;
    out[6] = bs->n_gterms;
    out[7] = bs->mixed_ok ? bs->n_sc : 0;
    return 0;
}

int amm_pme_create(amm_ctx *ctx, double alpha, int32_t nx, int32_t ny, int32_t nz, double Kc, const double *h_q,
                   int32_t *force_id) {
    if (!ctx || !h_q || !force_id) {
        amm_set_error("amm_pme_create: bad arguments");
        return 1;
    }
    if (!ctx->has_box) {
        amm_set_error("amm_pme_create: the context has no periodic box");
        return 1;
    }
    AMM_HIP(hipSetDevice(ctx->device));
    const int K[3] = {nx, ny, nz};
    PmeForce *pm = nullptr;
    if (amm_pme_create_impl(ctx, alpha, K, Kc, h_q, &pm)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_PME, pm);
    return 0;
}

int amm_pme_set_charges(amm_ctx *ctx, int32_t force_id, const double *h_q) {
    PmeForce *pm = amm_force_get<PmeForce>(ctx, force_id);
    if (!pm || !h_q) return 1;
    return amm_pme_set_charges_impl(ctx, pm, h_q);
}

int amm_pme_set_sliced(amm_ctx *ctx, int32_t force_id, int32_t on) {
    PmeForce *pm = amm_force_get<PmeForce>(ctx, force_id);
    if (!pm) return 1;
    return amm_pme_set_sliced_impl(pm, on);
}

int amm_force_eval(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_force, int32_t accumulate,
                   double *d_energy) {
    if (!ctx || force_id < 0 || force_id >= (int)ctx->forces.size() || !d_pos || !d_force) {
        amm_set_error("amm_force_eval: bad arguments");
        return 1;
    }
    if (!(ctx->opt_positions_private && d_pos == ctx->d_x)) ctx->pos_epoch++;     // a caller's positions may have changed in any way since the last call
    return amm_force_eval_dispatch(ctx, force_id, d_pos, d_force, accumulate, d_energy);
}

int amm_positions_changed(amm_ctx *ctx) {
    if (!ctx) return 1;
    ctx->pos_epoch++;
    return 0;
}

int amm_min_create(amm_ctx *ctx, int32_t memory, double max_step, int32_t force_input, const double *d_mass, double *d_scalars,
                   int32_t *min_id) {
    if (!ctx || !d_scalars || !min_id) {
        amm_set_error("amm_min_create: bad arguments");
        return 1;
    }
    int id = -1;
    if (amm_min_create_impl(ctx, memory, max_step, force_input, d_mass, d_scalars, &id)) return 1;
    *min_id = id;
    return 0;
}
int amm_min_release(amm_ctx *ctx, int32_t min_id) { return amm_min_release_impl(ctx, min_id); }
int amm_min_begin(amm_ctx *ctx, int32_t min_id, const double *d_x, const double *d_g) { return amm_min_begin_impl(ctx, min_id, d_x, d_g); }
int amm_min_advance(amm_ctx *ctx, int32_t min_id, const double *d_x, const double *d_g) {
    return amm_min_advance_impl(ctx, min_id, d_x, d_g);
}
int amm_min_trial(amm_ctx *ctx, int32_t min_id, double alpha, double *d_x_out) {
    if (ctx) ctx->pos_epoch++;            // (the output may be the bound position buffer: as amm_move)
    return amm_min_trial_impl(ctx, min_id, alpha, d_x_out);
}
int amm_min_scalars(amm_ctx *ctx, int32_t min_id, double out[8]) { return amm_min_scalars_impl(ctx, min_id, out); }
int amm_min_stats(amm_ctx *ctx, int32_t min_id, int64_t out[8]) { return amm_min_stats_impl(ctx, min_id, out); }
int amm_min_read(amm_ctx *ctx, int32_t min_id, int32_t what, double *h_out) { return amm_min_read_impl(ctx, min_id, what, h_out); }

int amm_kick(amm_ctx *ctx, double *d_v, const double *d_f, const double *d_f2, int32_t plus, const double *d_mass, double coef) {
    return amm_kick_impl(ctx, d_v, d_f, d_f2, plus, d_mass, coef);
}
int amm_move(amm_ctx *ctx, double *d_x, const double *d_v, double coef) {
    if (amm_move_impl(ctx, d_x, d_v, coef)) return 1;
    if (d_x == ctx->d_x && amm_vsite_place_impl(ctx, d_x)) return 1;     // (sites follow every update of the bound positions)
    ctx->pos_epoch++;
    return 0;
}
int amm_copy(amm_ctx *ctx, double *d_dst, const double *d_src) {
    if (amm_copy_impl(ctx, d_dst, d_src)) return 1;
    if (d_dst == ctx->d_x && amm_vsite_place_impl(ctx, d_dst)) return 1;
    ctx->pos_epoch++;
    return 0;
}

int amm_vsite_define(amm_ctx *ctx, int32_t n_sites, const int32_t *h_site, const int32_t *h_kind, const int32_t *h_parents,
                     const double *h_weights) {
    if (!ctx || n_sites < 0 || (n_sites > 0 && (!h_site || !h_kind || !h_parents || !h_weights))) {
        amm_set_error("amm_vsite_define: bad arguments");
        return 1;
    }
    return amm_vsite_define_impl(ctx, n_sites, h_site, h_kind, h_parents, h_weights);
}
int amm_vsite_place(amm_ctx *ctx, double *d_x) {
    if (!ctx || !d_x) {
        amm_set_error("amm_vsite_place: null argument");
        return 1;
    }
    if (amm_vsite_place_impl(ctx, d_x)) return 1;
    ctx->pos_epoch++;
    return 0;
}
int amm_vsite_spread(amm_ctx *ctx, const double *d_x, double *d_f) {
    if (!ctx || !d_x || !d_f) {
        amm_set_error("amm_vsite_spread: null argument");
        return 1;
    }
    return amm_vsite_spread_impl(ctx, d_x, d_f);
}
int amm_vsite_stats(amm_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return 1;
    return amm_vsite_stats_impl(ctx, out);
}
int amm_mvv(amm_ctx *ctx, const double *d_v, const double *d_m, double *d_out) { return amm_mvv_impl(ctx, d_v, d_m, d_out); }

int amm_expr_eval(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts,
                  const double *globals, int32_t n_globals, uint64_t seed, uint64_t counter, double *d_dst, double *d_sum) {
    if (!ctx || !code || (n_consts > 0 && !consts) || (n_globals > 0 && !globals) || (!d_dst && !d_sum)) {
        amm_set_error("amm_expr_eval: bad arguments");
        return 1;
    }
    if (d_dst) ctx->pos_epoch++;          // (the destination may be the position buffer, or alias it)
    return amm_expr_eval_impl(ctx, code, n_code, consts, n_consts, globals, n_globals, seed, counter, d_dst, d_sum);
}

int amm_expr_eval_scalar(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts, double *d_scalars,
                         int32_t n_scalars) {
    if (!ctx || !code || (n_consts > 0 && !consts) || !d_scalars) {
        amm_set_error("amm_expr_eval_scalar: bad arguments");
        return 1;
    }
    return amm_expr_eval_scalar_impl(ctx, code, n_code, consts, n_consts, d_scalars, n_scalars);
}

int amm_constraints_create(amm_ctx *ctx, const int32_t *h_pairs, const double *h_dist, int32_t n_constraints, double tolerance) {
    if (!ctx || (n_constraints > 0 && (!h_pairs || !h_dist)) || n_constraints < 0) {
        amm_set_error("amm_constraints_create: bad arguments");
        return 1;
    }
    AMM_HIP(hipSetDevice(ctx->device));
    // the new set first: a refused call leaves the previous set in force
    ConstraintSet *fresh = nullptr;
    if (amm_constraints_create_impl(ctx, h_pairs, h_dist, n_constraints, tolerance, &fresh)) return 1;
    if (ctx->constraints) amm_constraints_free(ctx->constraints);
    ctx->constraints = fresh;
    return 0;
}

int amm_constraints_set_tolerance(amm_ctx *ctx, double tolerance) {
    if (!ctx || !ctx->constraints) {
        amm_set_error("amm_constraints_set_tolerance: the context has no constraint set (amm_constraints_create)");
        return 1;
    }
    return amm_constraints_set_tolerance_impl(ctx->constraints, tolerance);
}

int amm_expr_define(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts,
                    const double *globals, int32_t n_globals, int32_t *expr_id) {
    if (!ctx || !code || n_code < 1 || !expr_id || (n_consts > 0 && !consts) || (n_globals > 0 && !globals)) {
        amm_set_error("amm_expr_define: bad arguments");
        return 1;
    }
    ExprDef e;
    e.code.assign(code, code + n_code);
    if (n_consts > 0) e.consts.assign(consts, consts + n_consts);
    if (n_globals > 0) e.globals.assign(globals, globals + n_globals);
    ctx->exprs.push_back(e);
    *expr_id = (int32_t)ctx->exprs.size() - 1;
    return 0;
}

int amm_bath_define(amm_ctx *ctx, double z, double kT, int32_t *bath_id) {
    if (!ctx || !bath_id || !(z >= 0.0 && z <= 1.0) || !(kT >= 0.0)) {
        amm_set_error("amm_bath_define: need 0 <= z <= 1 and kT >= 0");
        return 1;
    }
    BathDef b;
    b.z = z;
    b.kT = kT;
    ctx->baths.push_back(b);
    *bath_id = (int32_t)ctx->baths.size() - 1;
    return 0;
}

int amm_stock_define(amm_ctx *ctx, int32_t kind, double dt, double friction, double kT, int32_t *stock_id) {
    if (!ctx || !stock_id) {
        amm_set_error("amm_stock_define: null argument");
        return 1;
    }
    if (kind < AMM_STOCK_VERLET || kind > AMM_STOCK_BROWNIAN) {
        amm_set_error("amm_stock_define: unknown kind " + std::to_string(kind) + " (0 Verlet, 1 LangevinMiddle, 2 Langevin, 3 Brownian)");
        return 1;
    }
    if (!(friction >= 0.0) || !(kT >= 0.0)) {
        amm_set_error("amm_stock_define: the friction and kT must not be negative");
        return 1;
    }
    if (kind == AMM_STOCK_BROWNIAN && !(friction > 0.0)) {
        amm_set_error("amm_stock_define: a Brownian integrator needs a friction > 0");
        return 1;
    }
    if (!(dt == dt) || dt == 0.0) {
        amm_set_error("amm_stock_define: the step size must not be 0 (the velocities are differences of positions over it)");
        return 1;
    }
    StockDef sd;
    sd.kind = kind;
    sd.dt = dt;
    sd.friction = friction;
    sd.kT = kT;
    sd.a = exp(-friction * dt);
    sd.b = friction > 0.0 ? (1.0 - sd.a) / friction : dt;
    ctx->stocks.push_back(sd);
    *stock_id = (int32_t)ctx->stocks.size() - 1;
    return 0;
}

int amm_drude_step_define(amm_ctx *ctx, const int32_t *h_pairs, int32_t n_pairs, double dt, double friction, double kT, double drude_friction,
                          double drude_kT, double max_distance, int32_t *step_id) {
    if (!ctx || !step_id || (n_pairs > 0 && !h_pairs)) {
        amm_set_error("amm_drude_step_define: null argument");
        return 1;
    }
    int id = -1;
    if (amm_drude_step_define_impl(ctx, h_pairs, n_pairs, dt, friction, kT, drude_friction, drude_kT, max_distance, &id)) return 1;
    *step_id = id;
    return 0;
}

int amm_bath_define_nhl(amm_ctx *ctx, double h, double z, double kT, double Q, double friction, int32_t slot, int32_t *bath_id) {
    if (!ctx || !bath_id || !(z >= 0.0 && z <= 1.0) || !(kT >= 0.0) || !(Q > 0.0) || !(friction > 0.0) || slot < 0 || slot >= AMM_SLOT_X) {
        amm_set_error("amm_bath_define_nhl: need 0 <= z <= 1, kT >= 0, Q > 0, friction > 0 and a per-DOF buffer slot");
        return 1;
    }
    BathDef b;
    b.z = z;
    b.kT = kT;
    b.kind = 1;
    b.h = h;
    b.Q = Q;
    b.friction = friction;
    b.slot = slot;
    ctx->baths.push_back(b);
    *bath_id = (int32_t)ctx->baths.size() - 1;
    return 0;
}

int amm_bath_define_sin(amm_ctx *ctx, double h, double z, double kT, double Q2, double friction, int32_t slot_v2, int32_t *bath_id) {
    if (!ctx || !bath_id || !(z >= 0.0 && z <= 1.0) || !(kT >= 0.0) || !(Q2 > 0.0) || !(friction > 0.0) || slot_v2 < 0 || slot_v2 >= AMM_SLOT_X) {
        amm_set_error("amm_bath_define_sin: need 0 <= z <= 1, kT >= 0, Q2 > 0, friction > 0 and a per-DOF buffer slot");
        return 1;
    }
    BathDef b;
    b.z = z;
    b.kT = kT;
    b.kind = 2;
    b.h = h;
    b.Q = Q2;
    b.friction = friction;
    b.slot = slot_v2;
    ctx->baths.push_back(b);
    *bath_id = (int32_t)ctx->baths.size() - 1;
    return 0;
}

int amm_bath_define_regulated(amm_ctx *ctx, int32_t kind, int32_t split, double h, double z, double kT, double Q, double omega,
                              double friction, double alpha, double an, int32_t slot_v_eta, int32_t *bath_id) {
    if (!ctx || !bath_id || kind < 3 || kind > 6 || !(z >= 0.0 && z <= 1.0) || !(kT > 0.0) || !(Q > 0.0) || !(omega >= 0.0) ||
        !(friction > 0.0) || !(alpha > 0.0) || !(an > 0.0) || slot_v_eta < 0 || slot_v_eta >= AMM_SLOT_X) {
        amm_set_error("amm_bath_define_regulated: need kind 3..6, 0 <= z <= 1, kT > 0, Q > 0, omega >= 0, friction > 0, alpha > 0, "
                      "an > 0 and a per-DOF buffer slot");
        return 1;
    }
    BathDef b;
    b.kind = kind;
    b.split = split != 0;
    b.h = h;
    b.z = z;
    b.kT = kT;
    b.Q = Q;
    b.omega = omega;
    b.friction = friction;
    b.alpha = alpha;
    b.an = an;
    const double n = an / alpha;
    b.kfac = (n + 1.0) / (alpha * n);
    b.slot = slot_v_eta;
    ctx->baths.push_back(b);
    *bath_id = (int32_t)ctx->baths.size() - 1;
    return 0;
}

int amm_regulated_define(amm_ctx *ctx, int32_t on, double alpha, double an_kT) {
    if (!ctx || (on && !(alpha > 0.0 && an_kT > 0.0))) {
        amm_set_error("amm_regulated_define: need alpha > 0 and an_kT > 0");
        return 1;
    }
    ctx->reg.on = on != 0;
    ctx->reg.alpha = alpha;
    ctx->reg.an_kT = an_kT;
    return 0;
}

int amm_iso_define(amm_ctx *ctx, int32_t on, double LkT, double Q1, int32_t slot_v1) {
    if (!ctx || (on && (!(LkT > 0.0) || !(Q1 > 0.0) || slot_v1 < 0 || slot_v1 >= AMM_SLOT_X))) {
        amm_set_error("amm_iso_define: need LkT > 0, Q1 > 0 and a per-DOF buffer slot");
        return 1;
    }
    ctx->iso.on = on != 0;
    ctx->iso.LkT = LkT;
    ctx->iso.Q1 = Q1;
    ctx->iso.slot = slot_v1;
    return 0;
}

int amm_comm_unique_id(const char *rccl_path, uint8_t id[AMM_COMM_ID_BYTES]) {
    if (!id) {
        amm_set_error("amm_comm_unique_id: null output");
        return 1;
    }
    return amm_comm_unique_id_impl(rccl_path, id);
}
int amm_comm_init(amm_ctx *ctx, const char *rccl_path, const uint8_t id[AMM_COMM_ID_BYTES], int32_t rank, int32_t world) {
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world) {
        amm_set_error("amm_comm_init: bad arguments");
        return 1;
    }
    return amm_comm_init_impl(ctx, rccl_path, id, rank, world);
}
int amm_comm_destroy(amm_ctx *ctx) {
    if (!ctx) return 1;
    return amm_comm_destroy_impl(ctx);
}
int amm_comm_stats(amm_ctx *ctx, int64_t out[2]) {
    if (!ctx || !out) return 1;
    out[0] = ctx->comm_calls;
    out[1] = ctx->comm_doubles;
    return 0;
}
int amm_comm_allreduce(amm_ctx *ctx, double *d_buf, int64_t count) {
    if (!ctx || !d_buf || count < 0) {
        amm_set_error("amm_comm_allreduce: bad arguments");
        return 1;
    }
    return amm_comm_allreduce_impl(ctx, d_buf, (size_t)count);
}

int amm_expr_seed(amm_ctx *ctx, uint64_t seed) {
    if (!ctx) {
        amm_set_error("amm_expr_seed: null context");
        return 1;
    }
    ctx->expr_seed = seed;
    ctx->expr_counter = 0;
    return 0;
}

int amm_bind_state(amm_ctx *ctx, double *d_x, double *d_v, const double *d_mass) {
    if (!ctx || !d_x || !d_v || !d_mass) {
        amm_set_error("amm_bind_state: null argument");
        return 1;
    }
    ctx->d_x = d_x;
    ctx->d_v = d_v;
    ctx->d_mass = d_mass;
    ctx->slots[AMM_SLOT_X] = d_x;
    ctx->slots[AMM_SLOT_V] = d_v;
    return 0;
}
int amm_bind_buffer(amm_ctx *ctx, int32_t slot, double *d_buf) {
    if (slot < 0 || slot >= AMM_MAX_SLOTS) {
        amm_set_error("amm_bind_buffer: slot out of range");
        return 1;
    }
    ctx->slots[slot] = d_buf;
    return 0;
}
int amm_group_define(amm_ctx *ctx, int32_t group, int32_t slot, const int32_t *force_ids, int32_t n_forces) {
    if (!ctx || (n_forces > 0 && !force_ids) || n_forces < 0) {
        amm_set_error("amm_group_define: null argument");
        return 1;
    }
    if (group < 0 || group >= AMM_MAX_GROUPS || slot < 0 || slot >= AMM_MAX_SLOTS) {
        amm_set_error("amm_group_define: group/slot out of range");
        return 1;
    }
    for (int32_t k = 0; k < n_forces; ++k)
        if (force_ids[k] < 0 || force_ids[k] >= (int32_t)ctx->forces.size()) {
            amm_set_error("amm_group_define: unknown force id");
            return 1;
        }
    ctx->groups[group].slot = slot;
    ctx->groups[group].forces.assign(force_ids, force_ids + n_forces);
    return 0;
}

int amm_group_set_exchange(amm_ctx *ctx, int32_t group, int32_t mode) {
    if (!ctx || group < 0 || group >= AMM_MAX_GROUPS || (mode != AMM_EXCHANGE_REDUCE && mode != AMM_EXCHANGE_GATHER)) {
        amm_set_error("amm_group_set_exchange: bad group or mode");
        return 1;
    }
    ctx->groups[group].exchange = mode;
    return 0;
}
int amm_bind_exchange(amm_ctx *ctx, double *d_buf, int64_t n_doubles) {
    if (!ctx || (n_doubles > 0 && !d_buf) || n_doubles < 0) {
        amm_set_error("amm_bind_exchange: bad arguments");
        return 1;
    }
    ctx->d_xchg = d_buf;
    ctx->xchg_doubles = n_doubles;
    return 0;
}
int amm_exchange_pending(amm_ctx *ctx, int32_t *nf) {
    if (!ctx || !nf) return 1;
    *nf = ctx->pending.active ? ctx->pending.nf : 0;
    return 0;
}
int amm_exchange_finish(amm_ctx *ctx) {
    if (!ctx) return 1;
    return amm_exchange_finish_impl(ctx);
}

int amm_run_ops(amm_ctx *ctx, const amm_op *ops, int32_t n_ops, int32_t repeat) { return amm_run_ops_from(ctx, ops, n_ops, repeat, nullptr); }

// cursor != nullptr: resumable.  Starts at op *cursor of the unrolled program (repetition * n_ops + index) and runs to its end --
// or to the first exchanged evaluation whose exchange is the HOST's to make (no communicator of the library's own): then it returns 0
// with *cursor at the op to go on from and the exchange pending (the host all-gathers the chunks, calls amm_exchange_finish and
// calls again).  *cursor == repeat * n_ops on return: the program is through.  (The scheduler itself: run_ops.hip.)
int amm_run_ops_from(amm_ctx *ctx, const amm_op *ops, int32_t n_ops, int32_t repeat, int64_t *cursor) {
    if (!ctx) {
        amm_set_error("amm_run_ops: null context");
        return 1;
    }
    if (n_ops <= 0 || repeat <= 0) {        // an empty program: through before it starts
        if (cursor) *cursor = 0;
        return 0;
    }
    if (!ops) {
        amm_set_error("amm_run_ops: null ops");
        return 1;
    }
    return amm_run_ops_impl(ctx, ops, n_ops, repeat, cursor);
}

int amm_pair_get_stats(amm_ctx *ctx, int32_t force_id, amm_pair_stats *out) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf || !out) return 1;
    std::memset(out, 0, sizeof(*out));
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    out->n_evals = pf->n_evals;
    if (pf->free_space) {          // no grid, no list, no builds: its evaluations and its lanes per row
        out->lanes_per_atom = amm_free_lanes_per_row(pf->n);
        out->n_slice_atoms = pf->n;
        out->list_kind = 4;
        return 0;
    }
    PairForce *L = pf->host ? pf->host : pf;
    out->capacity = L->cap;
    out->lanes_per_atom = L->lpa;
    out->n_cells = L->grid.ncell;
    out->rlist = pf->rlist;
    out->n_slice_atoms = L->s_end - L->s_begin;
    out->shares_list = pf->host ? 1 : 0;
    out->list_kind = L->last_kind;
    out->tab_error = pf->tab_error;
    out->has_table = (pf->pc.tab.nint > 0 && pf->d_tab) ? 1 : 0;
    out->rode_along = pf->last_fused;
    out->chargeless = pf->last_chargeless;
    out->build_split = (L->cl && L->last_kind != 0) ? L->cl->split_parts : 0;
    out->has_site_table = (ctx->opt_site_tab && pf->d_tab_ss && pf->pc.tab.ss_first >= 0) ? 1 : 0;
    out->site_tab_error = pf->ss_error;
    out->n_rest_atoms = L->hybrid ? L->n_rest : 0;
    if (pf->small) {
        int cs[2];
        if (amm_small_group_stats(pf->small, cs)) return 1;
        out->n_candidates = cs[0];
        out->n_candidate_walks = cs[1];
    }
    if (L->last_kind >= 1 && L->cl && L->cl->built) {
        ClusterList *cl = L->cl;
        int flags[8];
        unsigned long long cnt[8];
        AMM_HIP(hipMemcpy(flags, cl->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
        AMM_HIP(hipMemcpy(cnt, cl->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
        out->capacity = cl->cap;
        out->lanes_per_atom = cl->lpa;
        out->n_cells = cl->grid.ncell;
        out->n_slice_atoms = 3 * (int64_t)(cl->c_end - cl->c_begin);
        out->n_builds = (int64_t)cnt[0];
        out->n_list_pairs = 9 * (int64_t)(pf->host ? cnt[2] : cnt[1]);      // atom pairs evaluated: nine per molecule-pair entry
        out->max_neighbors = flags[2];
        out->rlist_outer = L->desc.rc + L->skin;
        if (L->last_kind == 2 && L->rest && L->rest->built) {          // + the entries of the per-atom part
            AMM_HIP(hipMemcpy(cnt, L->rest->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
            out->n_list_pairs += (int64_t)(pf->host ? cnt[2] : cnt[1]);
        }
        return 0;
    }
    if (L->built) {
        int flags[8];
        unsigned long long cnt[8];
        AMM_HIP(hipMemcpy(flags, L->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
        AMM_HIP(hipMemcpy(cnt, L->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
        out->n_builds = (int64_t)cnt[0];
        out->n_outer_builds = (int64_t)cnt[4];
        out->n_outer_pairs = (int64_t)cnt[3];
        out->rlist_outer = L->desc.rc + L->skin_out;
        out->n_list_pairs = (int64_t)(pf->host ? cnt[2] : cnt[1]);   // a guest walks the front parts only
        out->max_neighbors = flags[2];
    }
    return 0;
}

int amm_pair_guest_factor(amm_ctx *ctx, int32_t force_id, double out[2]) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf || !out) {
        amm_set_error("amm_pair_guest_factor: null argument or not a pair force");
        return 1;
    }
    out[0] = pf->last_gfac;
    out[1] = pf->last_gunit ? 1.0 : 0.0;
    return 0;
}

int amm_pair_row_padding(amm_ctx *ctx, int32_t force_id, int64_t out[2]) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf || !out) {
        amm_set_error("amm_pair_row_padding: null argument or not a pair force");
        return 1;
    }
    PairForce *L = pf->host ? pf->host : pf;
    out[0] = out[1] = 0;
    if (pf->free_space) return 0;
    if (!(L->last_kind >= 1 && L->cl && L->cl->built)) return 0;       // per-atom rows: not reported
    long long v[2];
    if (amm_cluster_row_padding_impl(ctx, pf, v)) return 1;
    out[0] = v[0];
    out[1] = v[1];
    return 0;
}

int amm_pair_count_within(amm_ctx *ctx, int32_t force_id, const double *d_pos, double r_within, int64_t *count) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf || !d_pos || !count) {
        amm_set_error("amm_pair_count_within: null argument or not a pair force");
        return 1;
    }
    if (pf->free_space) {
        amm_set_error("amm_pair_count_within: a free-space pair force (AMM_FREE_SPACE) has no neighbour rows to count");
        return 1;
    }
    long long c = 0;
    PairForce *Lw = pf->host ? pf->host : pf;
    if (Lw->last_kind >= 1 && Lw->cl && Lw->cl->built) {
        if (amm_cluster_count_within_impl(ctx, pf, d_pos, r_within, &c)) return 1;
        if (Lw->last_kind == 2 && pf->rest && Lw->rest && Lw->rest->built) {
            long long c2 = 0;
            if (amm_pair_count_within_impl(ctx, pf->rest, d_pos, r_within, &c2)) return 1;
            c += c2;
        }
    } else if (amm_pair_count_within_impl(ctx, pf, d_pos, r_within, &c)) return 1;
    *count = (int64_t)c;
    return 0;
}

const char *amm_kernel_revision(void) { return amm_kernel_revision_impl(); }

int amm_pair_table_check(const amm_pair_desc *desc, double site_sigma, double site_eps, double site_q, int64_t out[8]) {
    if (!desc || !out) {
        amm_set_error("amm_pair_table_check: null argument");
        return 1;
    }
    long long v[8];
    if (amm_pair_table_check_impl(*desc, site_sigma, site_eps, site_q, v)) return 1;
    for (int k = 0; k < 8; ++k) out[k] = (int64_t)v[k];
    return 0;
}

int amm_set_outer_skin(amm_ctx *ctx, double skin_out) {
    ctx->skin_out = skin_out;
    return 0;
}

int amm_set_option(amm_ctx *ctx, const char *name, double value) {
    if (!ctx || !name) {
        amm_set_error("amm_set_option: null argument");
        return 1;
    }
    const std::string k(name);
    const int v = (int)value;
    if (k == "cluster") ctx->opt_cluster = v;
    else if (k == "hybrid") ctx->opt_hybrid = v;
    else if (k == "small_group") ctx->opt_small_group = v;
    else if (k == "mixed_terms") ctx->opt_mixed_terms = v;
    else if (k == "rest_skin_factor") ctx->opt_rest_skin_factor = value;
    else if (k == "tab") ctx->opt_tab = v;
    else if (k == "site_trips") ctx->site_trips = v != 0;
    else if (k == "lanes_per_row") ctx->opt_lpa = v;
    else if (k == "build_parts") ctx->opt_parts = v;
    else if (k == "build_split") ctx->opt_build_split = v;
    else if (k == "unroll") ctx->opt_unroll = v;
    else if (k == "dual_unroll") ctx->opt_dual_unroll = v;
    else if (k == "tab_block") ctx->opt_tab_bs = v;
    else if (k == "tab_dual_block") ctx->opt_tab_dual_bs = v;
    else if (k == "fuse_rows") ctx->opt_fuse_rows = v;
    else if (k == "row_phases") ctx->opt_row_phases = v;
    else if (k == "group_candidates") ctx->opt_group_candidates = v;
    else if (k == "positions_private") ctx->opt_positions_private = v;
    else if (k == "site_tab") ctx->opt_site_tab = v;
    else if (k == "terms_from") ctx->opt_terms_from = v;
    else if (k == "no_term_lanes") ctx->opt_no_term_lanes = v;
    else if (k == "fuse_epilogue") ctx->opt_fuse_epilogue = v;
    else if (k == "comm_timeout") ctx->opt_comm_timeout = value;
    else if (k == "spec_assign") ctx->opt_spec_assign = v;
    else if (k == "chargeless") ctx->opt_chargeless = v;
    else if (k == "state_exchange") ctx->opt_state_exchange = v;
    else if (k == "gb_lanes_per_row") {
        if (v < 0 || v > 64 || (v & (v - 1))) {
            amm_set_error("amm_set_option: gb_lanes_per_row is 0 (automatic) or a power of two up to 64");
            return 1;
        }
        ctx->opt_gb_lpr = v;
    }
    else if (k == "cgb_lanes_per_row") {
        if (v < 0 || v > 64 || (v & (v - 1))) {
            amm_set_error("amm_set_option: cgb_lanes_per_row is 0 (automatic) or a power of two up to 64");
            return 1;
        }
        ctx->opt_cgb_lpr = v;
    }
    else if (k == "hbond_chunks") {
        if (v < 0 || v > 512) {
            amm_set_error("amm_set_option: hbond_chunks is 0 (automatic) or 1 .. 512 column chunks per row");
            return 1;
        }
        ctx->opt_hbond_chunks = v;
    }
    else if (k == "hbond_compact") ctx->opt_hbond_compact = v != 0;
    else if (k == "many_capacity") {
        if (v < 64 || v > 4096 || v % 64 != 0) {
            amm_set_error("amm_set_option: many_capacity is a multiple of 64 from 64 to 4096 neighbours per row");
            return 1;
        }
        ctx->opt_many_capacity = v;
    }
    else if (k == "rmsd_blocks") {
        if (v < 0 || v > 1024) {
            amm_set_error("amm_set_option: rmsd_blocks is 0 (chosen from the selection's size), 1 (the single block) or 2 .. 1024 blocks");
            return 1;
        }
        ctx->opt_rmsd_blocks = v;
    }
    else {
        amm_set_error("amm_set_option: unknown option '" + k + "'");
        return 1;
    }
    return 0;
}

// ---- a box that changes (constant-pressure runs) --------------------------------------------------------------------------
// How far amm_set_box lets a kept grid squeeze a Verlet buffer before it chooses the cell counts again: half of the buffer the force
// would have in this box with cells to match.
static const double AMM_BOX_SKIN_KEEP = 0.5;
// ... and how far the density of list entries (rlist^3 / V) may grow beyond the first build's before the row capacities (1.5 x the
// longest row then + 32) are sized again: a quarter leaves a fifth for fluctuations.
static const double AMM_BOX_ROWS_GROW = 1.25;

// the largest list radius the cells of a kept grid admit in the context's box: neighbours within +-2 cells need cw >= radius / 2
static double grid_room(const amm_ctx *ctx, const CellGrid &g) {
    double room = 1.0e30;
    for (int k = 0; k < 3; ++k) room = std::min(room, 2.0 * ctx->box.L[k] / g.nc[k]);
    return room;
}
// the cell counts setup_grid / cluster_setup_grid would choose today for list radius `reach`
static bool grid_differs(const amm_ctx *ctx, const CellGrid &g, double reach) {
    for (int k = 0; k < 3; ++k) {
        int nc = (int)floor(ctx->box.L[k] / (0.5 * reach));
        nc = std::max(1, std::min(512, nc));
        if (nc != g.nc[k]) return true;
    }
    return false;
}
static bool box_within(const amm_ctx *ctx, const double L0[3], double tol) {
    for (int k = 0; k < 3; ++k)
        if (std::fabs(ctx->box.L[k] - L0[k]) > tol * L0[k]) return false;
    return true;
}

// the lists of the context follow ctx->box (amm_set_box, and its way back when a step of this fails)
static int box_apply(amm_ctx *ctx, bool &regrid, bool &waited) {
    const double V = ctx->box.L[0] * ctx->box.L[1] * ctx->box.L[2];
    // 1. every force's buffers as amm_pair_create would derive them in this box (a hybrid list's per-atom part asks for a multiple of
    // its parent's: the parent comes first in ctx->forces)
    for (auto &fo : ctx->forces) {
        if (fo.type != AMM_FORCE_PAIR || fo.pair()->free_space) continue;
        PairForce *pf = fo.pair();
        pair_derive_buffers(ctx, pf);
        if (pf->rest) pf->rest->skin_req = pf->skin * ctx->opt_rest_skin_factor;
    }
    // 2. list owners: keep the cell counts while the cells admit the list radius (the buffer gives way first, down to
    // AMM_BOX_SKIN_KEEP of it) and the capacities still fit the density; else choose them again -- a regrid: the list is dropped and
    // the next evaluation sizes and builds it as the first one did
    auto wait_once = [&]() -> int {
        if (!waited) AMM_HIP(hipStreamSynchronize(ctx->stream));
        waited = true;
        return 0;
    };
    for (auto &fo : ctx->forces) {
        if (fo.type != AMM_FORCE_PAIR || fo.pair()->host || fo.pair()->free_space) continue;
        PairForce *L = fo.pair();
        const bool dual = L->skin_out > L->skin * (1 + 1e-9);
        const double full_skin = L->skin;
        // per-atom rows
        {
            const double rgrid = dual ? L->rlist_out_build : L->rlist_build;
            const double room = grid_room(ctx, L->grid);
            const double skin_room = room - L->desc.rc - 2e-4 - 1e-9;
            bool again = false;
            if (!L->built) {
                // nothing is sized yet: the grid of a fresh context in this box; the per-cell arrays grow if they must
                if (grid_differs(ctx, L->grid, rgrid)) {
                    regrid = true;
                    if (amm_pair_setup_grid(ctx, L)) return 1;
                    again = L->grid.ncell > L->ncell_alloc;
                }
            } else if (dual != L->dual) again = true;     // the clamp took the outer buffer away, or gave it back: another kind of list
            else if (!box_within(ctx, L->built_L, 0.02) && grid_differs(ctx, L->grid, rgrid)) again = true;
            else if (rgrid > room && (dual || skin_room < 0.0 || skin_room < AMM_BOX_SKIN_KEEP * full_skin)) again = true;
            else if (L->rlist_build * L->rlist_build * L->rlist_build / V > AMM_BOX_ROWS_GROW * L->built_rows) again = true;
            if (again) {
                if (wait_once() || amm_pair_regrid(ctx, L)) return 1;
                regrid = true;
            } else {
                if (L->built && rgrid > room) L->skin = L->skin_out = skin_room;
                for (int k = 0; k < 3; ++k) {
                    L->grid.cw[k] = ctx->box.L[k] / L->grid.nc[k];
                    L->grid.inv_cw[k] = L->grid.nc[k] / ctx->box.L[k];
                }
            }
        }
        // molecule rows (their cells are wider by the molecules' extent)
        if (L->cl) {
            ClusterList *cl = L->cl;
            const double room = grid_room(ctx, cl->grid) - 2.0 * cl->rext;
            const double skin_room = room - L->desc.rc - 2e-4 - 1e-9;
            bool again = !cl->built;        // (a first build that failed: start over)
            if (!again && !box_within(ctx, cl->built_L, 0.02) && grid_differs(ctx, cl->grid, L->rlist_build + 2.0 * cl->rext)) again = true;
            if (!again && L->rlist_build > room && (skin_room < 0.0 || skin_room < AMM_BOX_SKIN_KEEP * full_skin)) again = true;
            if (!again && L->rlist_build * L->rlist_build * L->rlist_build / V > AMM_BOX_ROWS_GROW * cl->built_rows) again = true;
            if (again) {
                if (wait_once()) return 1;
                amm_cluster_free(cl);
                L->cl = nullptr;
                L->force_rebuild_c = false;
                regrid = true;
            } else if (L->rlist_build > room) {
                L->skin = L->skin_out = std::min(L->skin, skin_room);
            }
        }
        if (L->skin != full_skin) {
            const double reach = ((L->desc.flags & AMM_GUARD_RC0) && L->desc.rc0 > 0.0) ? std::min(L->desc.rc, L->desc.rc0) : L->desc.rc;
            L->rlist = reach + L->skin;
            L->rlist_build = L->rlist + 2e-4;
            L->rlist_out_build = reach + L->skin_out + 2e-4;
        }
    }
    // 3. shared lists, as amm_pair_share_list left them
    for (auto &fo : ctx->forces)
        if (fo.type == AMM_FORCE_PAIR && fo.pair()->host) {
            PairForce *g = fo.pair(), *h = g->host;
            g->rlist_build = std::min(g->rlist_build, h->desc.rc + std::min(g->skin, h->skin) + 2e-4);
            share_buffers(g, h);
        }
    // 4. nothing made for the old box survives: lists are rebuilt by their next evaluation, sorted copies gathered again, the
    // displacement triggers start from the positions of that rebuild, candidate sets start over
    for (auto &fo : ctx->forces) {
        if (fo.type != AMM_FORCE_PAIR || fo.pair()->free_space) continue;
        PairForce *pf = fo.pair();
        pf->a_sorted_for = nullptr;
        pf->a_sorted_epoch = pf->checked_epoch = pf->pre_epoch = -1;
        if (pf->built) pf->force_rebuild = true;
        if (pf->cl) amm_cluster_rebox(ctx, pf);
        amm_small_group_forget(pf->small);
    }
    ctx->n_watched = 0;
    ctx->pos_epoch++;
    return 0;
}

int amm_set_box(amm_ctx *ctx, const double h_box[3]) {
    if (!ctx || !h_box) {
        amm_set_error("amm_set_box: null argument");
        return 1;
    }
    for (int k = 0; k < 3; ++k)
        if (!(h_box[k] > 0.0)) {
            amm_set_error("amm_set_box: box edges must be positive (orthorhombic periodic box)");
            return 1;
        }
    if (!ctx->has_box) {
        amm_set_error("amm_set_box: the context has no periodic box");
        return 1;
    }
    if (ctx->world > 1 || ctx->pending.active) {
        amm_set_error("amm_set_box: a context that is one rank of several keeps the box it was created with");
        return 1;
    }
    for (auto &fo : ctx->forces)
        if (fo.type == AMM_FORCE_PAIR && !fo.pair()->free_space)
            for (int k = 0; k < 3; ++k)
                if (fo.pair()->desc.rc > 0.5 * h_box[k] * (1 + 1e-12)) {
                    amm_set_error("pair cutoff exceeds half the box edge (minimum image needs rc <= L/2)");
                    return 1;           // (nothing was touched: the old box stays in force)
                }
    const Box old = ctx->box;
    for (int k = 0; k < 3; ++k) {
        ctx->box.L[k] = h_box[k];
        ctx->box.invL[k] = 1.0 / h_box[k];
    }
    bool regrid = false, waited = false;
    if (box_apply(ctx, regrid, waited)) {
        // a wait or an allocation failed on the way: back to the old box (lists already dropped are built again by their next
        // evaluation), with the error of the first failure
        const std::string why = amm_last_error();
        bool r2 = false, w2 = false;
        ctx->box = old;
        (void)box_apply(ctx, r2, w2);
        amm_set_error(why);
        return 1;
    }
    ctx->box_changes++;
    if (regrid) ctx->box_regrids++;
    if (waited) ctx->box_waits++;
    return 0;
}

int amm_box_stats(amm_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return 1;
    out[0] = ctx->box_changes;
    out[1] = ctx->box_regrids;
    out[2] = ctx->box_waits;
    out[3] = 0;
    return 0;
}

int amm_mol_define(amm_ctx *ctx, const int32_t *h_ptr, const int32_t *h_atoms, int32_t n_mol) {
    if (!ctx || !h_ptr || !h_atoms) {
        amm_set_error("amm_mol_define: null argument");
        return 1;
    }
    return amm_mol_define_impl(ctx, h_ptr, h_atoms, n_mol);
}

int amm_mol_scale(amm_ctx *ctx, double *d_x, double *d_x_saved, const double scale[3]) {
    if (!ctx || !d_x || !scale) {
        amm_set_error("amm_mol_scale: null argument");
        return 1;
    }
    if (!ctx->has_box) {
        amm_set_error("amm_mol_scale: the context has no periodic box");
        return 1;
    }
    return amm_mol_scale_impl(ctx, d_x, d_x_saved, scale);
}

int amm_run_stats(amm_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return 1;
    out[0] = ctx->n_epilogues;
    out[1] = ctx->n_copies_current;
    out[2] = ctx->n_state_exchanges;
    out[3] = ctx->n_sched;
    return 0;
}

int amm_run_rule_stats(amm_ctx *ctx, int64_t out[8]) {
    if (!ctx || !out) return 1;
    for (int i = 0; i < 7; ++i) out[i] = ctx->n_rule[i];
    out[7] = ctx->n_plan_offers;
    return 0;
}

int amm_exchange_per(amm_ctx *ctx, int32_t *per) {
    if (!ctx || !per) return 1;
    *per = amm_slice_per(ctx->n, ctx->world);
    return 0;
}

int amm_set_fuse_inner(amm_ctx *ctx, int32_t on) {
    ctx->fuse_inner = on != 0;
    return 0;
}

int amm_profile_enable(amm_ctx *ctx, int32_t on) {
    ctx->profile = on != 0;
    ctx->profile_only = on < 0 ? -on - 1 : -1;
    return 0;
}

int amm_profile_read(amm_ctx *ctx, int32_t force_id, int64_t *n_launches, double *total_ms) {
    PairForce *pf = amm_force_get<PairForce>(ctx, force_id);
    if (!pf) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    double tot = 0.0;
    for (size_t k = 0; k + 1 < pf->ev_used; k += 2) {
        float ms = 0.f;
        AMM_HIP(hipEventElapsedTime(&ms, pf->ev[k], pf->ev[k + 1]));
        tot += ms;
    }
    if (n_launches) *n_launches = (int64_t)(pf->ev_used / 2);
    pf->ev_used = 0;
    // hybrid lists: an evaluation is two launches -- the molecule rows (timed above) and the per-atom part kept by the hidden child,
    // whose time belongs to the same evaluations (the launch count stays the parent's)
    if (pf->rest) {
        PairForce *rc = pf->rest;
        for (size_t k = 0; k + 1 < rc->ev_used; k += 2) {
            float ms = 0.f;
            AMM_HIP(hipEventElapsedTime(&ms, rc->ev[k], rc->ev[k + 1]));
            tot += ms;
        }
        rc->ev_used = 0;
    }
    if (total_ms) *total_ms = tot;
    return 0;
}

}  // extern "C"
