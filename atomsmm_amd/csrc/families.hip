// atomsmm_amd/csrc/families.hip -- the table of force families (amm_ctx.h: ForceFamily) and everything derived from it: the typed lookup
// with its refusals, registration, release and the dispatch of an evaluation; then the extern "C" entry points of the families whose
// implementation is a .hip file of its own (term expressions, collective variables, compound bonds, generalized Born, CMAP, custom
// generalized Born, hydrogen bonds, many-particle sets, RMSD, Gay-Berne ellipsoids, Drude oscillators).
#include <algorithm>
#include <cstring>

#include "amm_ctx.h"
#include "term_expr_vm.h"

// the families' own eval and free functions behind the table's one signature
template <class T, auto Eval> static int eval_as(amm_ctx *ctx, void *obj, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    return Eval(ctx, static_cast<T *>(obj), d_pos, d_force, accumulate, d_energy);
}
template <class T, auto Free> static void free_as(void *obj) { Free(static_cast<T *>(obj)); }
static int pair_eval(amm_ctx *ctx, PairForce *pf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    return amm_pair_eval_impl(ctx, pf, d_pos, d_force, accumulate, d_energy);      // (no guest, no exchange)
}
static int released_eval(amm_ctx *, void *, const double *, double *, int, double *) {
    amm_set_error("evaluation of a released force id");
    return 1;
}
static void released_free(void *) {}

// One row per AMM_FORCE_* value (a released id and the fourteen families), in the enum's order: noun phrase, tag, entry points, bad-id wording, single rank, eval, free.
const ForceFamily &amm_family(int type) {
    static const ForceFamily rows[AMM_FORCE_TYPES] = {
        {"a released id", "AMM_FORCE_RELEASED", "none", "released force id", false, released_eval, released_free},
        {"a pair force", "AMM_FORCE_PAIR", "amm_pair_*", "invalid pair force id", false,
         eval_as<PairForce, pair_eval>, free_as<PairForce, amm_pair_free>},
        {"a bond-list set", "AMM_FORCE_BONDED", "amm_bonded_*", "invalid bonded force id", false,
         eval_as<BondedSet, amm_bonded_eval_impl>, free_as<BondedSet, amm_bonded_free>},
        {"a PME force", "AMM_FORCE_PME", "amm_pme_*", "not a PME force id", false,
         eval_as<PmeForce, amm_pme_eval_impl>, free_as<PmeForce, amm_pme_free>},
        // (not single_rank: the library runs term expressions on a slice's context; it is the engine that refuses them on several ranks)
        {"a term-expression force", "AMM_FORCE_TERM_EXPR", "amm_term_expr_*", "not a term-expression force id", false,
         eval_as<TermExprForce, amm_term_expr_eval_impl>, free_as<TermExprForce, amm_term_expr_free>},
        {"a collective-variable force", "AMM_FORCE_CV", "amm_cv_*", "not the id of a collective-variable force (AMM_FORCE_CV)", true,
         eval_as<CvForce, amm_cv_eval_impl>, free_as<CvForce, amm_cv_free>},
        {"a compound-bond force", "AMM_FORCE_COMPOUND", "amm_compound_*", "not the id of a compound-bond force (AMM_FORCE_COMPOUND)", true,
         eval_as<CompoundForce, amm_compound_eval_impl>, free_as<CompoundForce, amm_compound_free>},
        {"a generalized-Born force", "AMM_FORCE_GB", "amm_gb_*", "not the id of a generalized-Born force (AMM_FORCE_GB)", true,
         eval_as<GbForce, amm_gb_eval_impl>, free_as<GbForce, amm_gb_free>},
        {"a CMAP force", "AMM_FORCE_CMAP", "amm_cmap_*", "not the id of a CMAP force (AMM_FORCE_CMAP)", true,
         eval_as<CmapForce, amm_cmap_eval_impl>, free_as<CmapForce, amm_cmap_free>},
        {"a custom generalized-Born force", "AMM_FORCE_CUSTOM_GB", "amm_custom_gb_*", "not the id of a custom generalized-Born force (AMM_FORCE_CUSTOM_GB)", true,
         eval_as<CustomGbForce, amm_custom_gb_eval_impl>, free_as<CustomGbForce, amm_custom_gb_free>},
        {"a hydrogen-bond force", "AMM_FORCE_HBOND", "amm_hbond_*", "not the id of a hydrogen-bond force (AMM_FORCE_HBOND)", true,
         eval_as<HbondForce, amm_hbond_eval_impl>, free_as<HbondForce, amm_hbond_free>},
        {"a many-particle force", "AMM_FORCE_MANY_PARTICLE", "amm_many_*", "not the id of a many-particle force (AMM_FORCE_MANY_PARTICLE)", true,
         eval_as<ManyForce, amm_many_eval_impl>, free_as<ManyForce, amm_many_free>},
        {"an RMSD force", "AMM_FORCE_RMSD", "amm_rmsd_*", "not the id of an RMSD force (AMM_FORCE_RMSD)", true,
         eval_as<RmsdForce, amm_rmsd_eval_impl>, free_as<RmsdForce, amm_rmsd_free>},
        {"a Gay-Berne force", "AMM_FORCE_GAYBERNE", "amm_gayberne_*", "not the id of a Gay-Berne force (AMM_FORCE_GAYBERNE)", true,
         eval_as<GayBerneForce, amm_gayberne_eval_impl>, free_as<GayBerneForce, amm_gayberne_free>},
        {"a Drude force", "AMM_FORCE_DRUDE", "amm_drude_*", "not the id of a Drude force (AMM_FORCE_DRUDE)", true,
         eval_as<DrudeForce, amm_drude_eval_impl>, free_as<DrudeForce, amm_drude_free>},
    };
    return rows[type];
}

// one force of any type (also the members of a group: run_ops.hip)
int amm_force_eval_dispatch(amm_ctx *ctx, int force_id, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const ForceObj &f = ctx->forces[force_id];
    return amm_family(f.type).eval(ctx, f.obj, d_pos, d_force, accumulate, d_energy);
}

int amm_force_register(amm_ctx *ctx, int type, void *obj) {
    ForceObj fo;
    fo.type = type;
    fo.obj = obj;
    ctx->forces.push_back(fo);
    return (int)ctx->forces.size() - 1;
}

void *amm_force_lookup(amm_ctx *ctx, int id, int type, const char *who) {
    const bool known = ctx && id >= 0 && id < (int)ctx->forces.size();
    if (known && ctx->forces[id].type == type) return ctx->forces[id].obj;
    std::string msg = (who ? std::string(who) + ": " : std::string()) + amm_family(type).bad_id;
    if (known && ctx->forces[id].type != AMM_FORCE_RELEASED) {
        const ForceFamily &owner = amm_family(ctx->forces[id].type);
        msg += ": force " + std::to_string(id) + " is " + owner.noun + " (" + owner.tag + ": " + owner.prefix + ")";
    }
    amm_set_error(msg);
    return nullptr;
}

// A force that the host has replaced (parameter offsets rebuild the exception terms, groups are merged anew, a Context goes away): its
// device arrays are freed, no group lists it any more and the id stays retired.
int amm_force_release(amm_ctx *ctx, int id, int type, const char *who) {
    void *obj = amm_force_lookup(ctx, id, type, who);
    if (!obj) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));            // nothing in flight may still read it
    for (int g = 0; g < AMM_MAX_GROUPS; ++g) {
        std::vector<int> &m = ctx->groups[g].forces;
        m.erase(std::remove(m.begin(), m.end(), id), m.end());
    }
    amm_family(type).free(obj);
    ctx->forces[id] = ForceObj();
    return 0;
}

extern "C" {

// Custom{Bond,Angle,Torsion,External}Force(any energy text): the compiled text (atomsmm_amd/expr.py: compile_term), the terms' atoms
// and their parameters, parameter-major
int amm_term_expr_create(amm_ctx *ctx, int32_t kind, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst,
                         const double *globals, int32_t nglobal, const int32_t *h_idx, const double *h_params, int32_t n_terms,
                         int32_t n_params, int32_t periodic, int32_t *force_id) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_term_expr_create: " + what);
        return 1;
    };
    if (!ctx || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals) || n_terms < 0 || (n_terms > 0 && !h_idx)) return fail("null argument");
    if (kind < AMM_TERM_BOND || kind > AMM_TERM_EXTERNAL) return fail("unknown kind " + std::to_string(kind));
    if (n_params < 0 || n_params > AMM_TERM_MAX_PARAMS) return fail(std::to_string(n_params) + " per-term parameters (limit " + std::to_string(AMM_TERM_MAX_PARAMS) + ")");
    if (n_params > 0 && n_terms > 0 && !h_params) return fail("null parameter array");
    if (periodic && kind == AMM_TERM_EXTERNAL) return fail("an external term reads raw coordinates: it is never periodic");
    if (periodic && !ctx->has_box) return fail("periodic terms, but the context has no periodic box");
    if (amm_expr_program_validate("amm_term_expr_create", code, ncode, nconst, nglobal, kind == AMM_TERM_EXTERNAL ? 3 : 1, n_params)) return 1;
    for (int t = 0; t < n_terms; ++t)
        for (int r = 0; r < amm_term_arity(kind); ++r) {
            const int a = h_idx[(size_t)t * 4 + r];
            if (a < 0 || a >= ctx->n) return fail("atom index " + std::to_string(a) + " of term " + std::to_string(t) + " is out of range");
        }
    AMM_HIP(hipSetDevice(ctx->device));
    TermExprForce *tf = new TermExprForce();
    tf->kind = kind;
    tf->periodic = periodic ? 1 : 0;
    tf->n_terms = n_terms;
    tf->n_params = n_params;
    tf->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    if (amm_term_expr_build(ctx, tf, h_idx, h_params)) {
        amm_term_expr_free(tf);
        return 1;
    }
    *force_id = amm_force_register(ctx, AMM_FORCE_TERM_EXPR, tf);
    return 0;
}

int amm_term_expr_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    TermExprForce *tf = amm_force_get<TermExprForce>(ctx, force_id, "amm_term_expr_set_globals");
    if (!tf) return 1;
    return tf->prog.set_globals(ctx, "amm_term_expr_set_globals", globals, nglobal);
}

int amm_term_expr_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_terms, int32_t n_params) {
    TermExprForce *tf = amm_force_get<TermExprForce>(ctx, force_id, "amm_term_expr_set_params");
    if (!tf) return 1;
    if (n_terms != tf->n_terms || n_params != tf->n_params || ((size_t)n_terms * n_params > 0 && !h_params)) {
        amm_set_error("amm_term_expr_set_params: the force has " + std::to_string(tf->n_terms) + " terms of " + std::to_string(tf->n_params) +
                      " parameters, " + std::to_string(n_terms) + " x " + std::to_string(n_params) + " given");
        return 1;
    }
    return amm_term_expr_upload_params(ctx, tf, h_params);
}

int amm_term_expr_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_TERM_EXPR, "amm_term_expr_release"); }

// CustomCVForce(any energy text): the compiled text (atomsmm_amd/expr.py: compile_cv) and the inner forces, one per collective variable
int amm_cv_create(amm_ctx *ctx, const int32_t *inner_ids, int32_t n_cv, int32_t n_deriv, const int32_t *code, int32_t ncode,
                  const double *consts, int32_t nconst, const double *globals, int32_t nglobal, int32_t *force_id) {
    if (!ctx || !inner_ids || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals)) {
        amm_set_error("amm_cv_create: null argument");
        return 1;
    }
    CvForce *cv = nullptr;
    if (amm_cv_create_impl(ctx, inner_ids, n_cv, n_deriv, code, ncode, consts, nconst, globals, nglobal, &cv)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_CV, cv);
    return 0;
}

int amm_cv_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    CvForce *cv = amm_force_get<CvForce>(ctx, force_id, "amm_cv_set_globals");
    return cv ? amm_cv_set_globals_impl(ctx, cv, globals, nglobal) : 1;
}

int amm_cv_set_variables(amm_ctx *ctx, int32_t force_id, const double *values, int32_t n_deriv) {
    CvForce *cv = amm_force_get<CvForce>(ctx, force_id, "amm_cv_set_variables");
    return cv ? amm_cv_set_variables_impl(ctx, cv, values, n_deriv) : 1;
}

int amm_cv_values(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out) {
    CvForce *cv = amm_force_get<CvForce>(ctx, force_id, "amm_cv_values");
    if (!cv) return 1;
    if (!d_pos || !h_out) {
        amm_set_error("amm_cv_values: null argument");
        return 1;
    }
    return amm_cv_values_impl(ctx, cv, d_pos, h_out);
}

int amm_cv_energy_derivative(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_out) {
    CvForce *cv = amm_force_get<CvForce>(ctx, force_id, "amm_cv_energy_derivative");
    if (!cv) return 1;
    if (!d_pos || !d_out) {
        amm_set_error("amm_cv_energy_derivative: null argument");
        return 1;
    }
    return amm_cv_energy_derivative_impl(ctx, cv, d_pos, d_out);
}

int amm_cv_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_CV, "amm_cv_release"); }

// CustomCompoundBondForce / CustomCentroidBondForce(any energy text): the compiled text and its variable table
// (atomsmm_amd/expr.py: compile_compound), the bonds' particles (or groups) and parameters, and for centroid bonds the groups
int amm_compound_create(amm_ctx *ctx, int32_t n_slots, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst,
                        const double *globals, int32_t nglobal, const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars,
                        const int32_t *h_idx, const double *h_params, int32_t n_bonds, int32_t n_params, int32_t periodic,
                        const int32_t *group_ptr, const int32_t *group_atoms, const double *group_weights, int32_t n_groups,
                        int32_t *force_id) {
    if (!ctx || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals) || (n_vars > 0 && (!var_kinds || !var_slots)) ||
        (n_bonds > 0 && !h_idx)) {
        amm_set_error("amm_compound_create: null argument");
        return 1;
    }
    CompoundForce *cf = nullptr;
    if (amm_compound_create_impl(ctx, n_slots, code, ncode, consts, nconst, globals, nglobal, var_kinds, var_slots, n_vars, h_idx, h_params,
                                 n_bonds, n_params, periodic, group_ptr, group_atoms, group_weights, n_groups, &cf))
        return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_COMPOUND, cf);
    return 0;
}

int amm_compound_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    CompoundForce *cf = amm_force_get<CompoundForce>(ctx, force_id, "amm_compound_set_globals");
    return cf ? amm_compound_set_globals_impl(ctx, cf, globals, nglobal) : 1;
}

int amm_compound_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_bonds, int32_t n_params) {
    CompoundForce *cf = amm_force_get<CompoundForce>(ctx, force_id, "amm_compound_set_params");
    return cf ? amm_compound_set_params_impl(ctx, cf, h_params, n_bonds, n_params) : 1;
}

int amm_compound_set_weights(amm_ctx *ctx, int32_t force_id, const double *weights, int32_t n_members) {
    CompoundForce *cf = amm_force_get<CompoundForce>(ctx, force_id, "amm_compound_set_weights");
    return cf ? amm_compound_set_weights_impl(ctx, cf, weights, n_members) : 1;
}

int amm_compound_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_COMPOUND, "amm_compound_release"); }

// GBSAOBCForce in free space (csrc/gb.hip): addParticle(charge, radius, scale) x n, the two dielectrics, the surface-area energy and
// the cutoff (rc <= 0: NoCutoff)
int amm_gb_create(amm_ctx *ctx, const double *h_q, const double *h_radius, const double *h_scale, double eps_in, double eps_out,
                  double sa_energy, double rc, int32_t *force_id) {
    if (!ctx || !h_q || !h_radius || !h_scale || !force_id) {
        amm_set_error("amm_gb_create: null argument");
        return 1;
    }
    AMM_HIP(hipSetDevice(ctx->device));
    GbForce *gb = nullptr;
    if (amm_gb_create_impl(ctx, h_q, h_radius, h_scale, eps_in, eps_out, sa_energy, rc, &gb)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_GB, gb);
    return 0;
}

int amm_gb_set_params(amm_ctx *ctx, int32_t force_id, const double *h_q, const double *h_radius, const double *h_scale, double eps_in,
                      double eps_out, double sa_energy, double rc) {
    GbForce *gb = amm_force_get<GbForce>(ctx, force_id, "amm_gb_set_params");
    return gb ? amm_gb_set_params_impl(ctx, gb, h_q, h_radius, h_scale, eps_in, eps_out, sa_energy, rc) : 1;
}

int amm_gb_born_radii(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out) {
    GbForce *gb = amm_force_get<GbForce>(ctx, force_id, "amm_gb_born_radii");
    if (!gb) return 1;
    if (!d_pos || !h_out) {
        amm_set_error("amm_gb_born_radii: null argument");
        return 1;
    }
    return amm_gb_born_radii_impl(ctx, gb, d_pos, h_out);
}

int amm_gb_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_GB, "amm_gb_release"); }

// CMAPTorsionForce (csrc/cmap.hip): addMap x n_maps as the bicubic coefficients of atomsmm_amd/tables.py (cmap_coefficients),
// addTorsion x n_terms as a map index and eight atoms each
int amm_cmap_create(amm_ctx *ctx, int32_t n_maps, const int32_t *h_sizes, const double *h_coeffs, const int32_t *h_map_of_term,
                    const int32_t *h_idx, int32_t n_terms, int32_t periodic, int32_t *force_id) {
    if (!ctx || !force_id || (n_maps > 0 && (!h_sizes || !h_coeffs)) || (n_terms > 0 && (!h_map_of_term || !h_idx))) {
        amm_set_error("amm_cmap_create: null argument");
        return 1;
    }
    CmapForce *cm = nullptr;
    if (amm_cmap_create_impl(ctx, n_maps, h_sizes, h_coeffs, h_map_of_term, h_idx, n_terms, periodic, &cm)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_CMAP, cm);
    return 0;
}

int amm_cmap_set_params(amm_ctx *ctx, int32_t force_id, const double *h_coeffs, const int32_t *h_map_of_term, int32_t n_maps, int32_t n_terms) {
    CmapForce *cm = amm_force_get<CmapForce>(ctx, force_id, "amm_cmap_set_params");
    return cm ? amm_cmap_set_params_impl(ctx, cm, h_coeffs, h_map_of_term, n_maps, n_terms) : 1;
}

int amm_cmap_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_CMAP, "amm_cmap_release"); }

// CustomGBForce in free space (csrc/custom_gb.hip): the programs of atomsmm_amd/expr.py (compile_custom_gb) -- the computed values',
// then the energy terms', concatenated -- the per-particle parameters, parameter-major, the exclusions and the cutoff (rc <= 0: NoCutoff)
int amm_custom_gb_create(amm_ctx *ctx, int32_t n_params, int32_t n_values, int32_t n_terms, const int32_t *types, const int32_t *code,
                         const int32_t *code_ptr, const double *consts, const int32_t *const_ptr, const double *globals, int32_t nglobal,
                         const double *h_params, const int32_t *h_excl, int32_t n_excl, double rc, int32_t *force_id) {
    const bool programs = n_values + n_terms > 0;
    if (!ctx || !force_id || !code_ptr || !const_ptr || (programs && (!types || !code)) || (nglobal > 0 && !globals) || (n_params > 0 && !h_params) ||
        (n_excl > 0 && !h_excl) || n_excl < 0) {
        amm_set_error("amm_custom_gb_create: null argument");
        return 1;
    }
    if (programs && const_ptr[n_values + n_terms] > 0 && !consts) {
        amm_set_error("amm_custom_gb_create: null argument");
        return 1;
    }
    AMM_HIP(hipSetDevice(ctx->device));
    CustomGbForce *cg = nullptr;
    if (amm_custom_gb_create_impl(ctx, n_params, n_values, n_terms, types, code, code_ptr, consts, const_ptr, globals, nglobal, h_params, h_excl,
                                  n_excl, rc, &cg))
        return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_CUSTOM_GB, cg);
    return 0;
}

int amm_custom_gb_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_params, int32_t n_atoms) {
    CustomGbForce *cg = amm_force_get<CustomGbForce>(ctx, force_id, "amm_custom_gb_set_params");
    return cg ? amm_custom_gb_set_params_impl(ctx, cg, h_params, n_params, n_atoms) : 1;
}

int amm_custom_gb_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    CustomGbForce *cg = amm_force_get<CustomGbForce>(ctx, force_id, "amm_custom_gb_set_globals");
    return cg ? amm_custom_gb_set_globals_impl(ctx, cg, globals, nglobal) : 1;
}

int amm_custom_gb_set_tables(amm_ctx *ctx, int32_t force_id, int32_t n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                             const int32_t *offsets, const double *data, int32_t n_data) {
    CustomGbForce *cg = amm_force_get<CustomGbForce>(ctx, force_id, "amm_custom_gb_set_tables");
    return cg ? amm_custom_gb_set_tables_impl(ctx, cg, n_tables, kinds, dims, ranges, offsets, data, n_data) : 1;
}

int amm_custom_gb_values(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out) {
    CustomGbForce *cg = amm_force_get<CustomGbForce>(ctx, force_id, "amm_custom_gb_values");
    if (!cg) return 1;
    if (!d_pos || !h_out) {
        amm_set_error("amm_custom_gb_values: null argument");
        return 1;
    }
    return amm_custom_gb_values_impl(ctx, cg, d_pos, h_out);
}

int amm_custom_gb_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_CUSTOM_GB, "amm_custom_gb_release"); }

// CustomHbondForce(any energy text) (csrc/hbond.hip): the compiled text and its variable table (atomsmm_amd/expr.py: compile_hbond),
// the donors' and acceptors' particles and parameters, the excluded (donor, acceptor) pairs, the cutoff (rc <= 0: NoCutoff) and
// whether displacements take the minimum image
int amm_hbond_create(amm_ctx *ctx, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst, const double *globals, int32_t nglobal,
                     const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars, const int32_t *h_donors, int32_t n_donors,
                     const int32_t *h_acceptors, int32_t n_acceptors, const double *h_donor_params, int32_t n_donor_params,
                     const double *h_acceptor_params, int32_t n_acceptor_params, const int32_t *h_excl, int32_t n_excl, double rc, int32_t periodic,
                     int32_t *force_id) {
    if (!ctx || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals) || (n_vars > 0 && (!var_kinds || !var_slots)) ||
        (n_donors > 0 && !h_donors) || (n_acceptors > 0 && !h_acceptors) || (n_excl > 0 && !h_excl)) {
        amm_set_error("amm_hbond_create: null argument");
        return 1;
    }
    HbondForce *hb = nullptr;
    if (amm_hbond_create_impl(ctx, code, ncode, consts, nconst, globals, nglobal, var_kinds, var_slots, n_vars, h_donors, n_donors, h_acceptors,
                              n_acceptors, h_donor_params, n_donor_params, h_acceptor_params, n_acceptor_params, h_excl, n_excl, rc, periodic, &hb))
        return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_HBOND, hb);
    return 0;
}

int amm_hbond_set_params(amm_ctx *ctx, int32_t force_id, const double *h_donor_params, int32_t n_donors, int32_t n_donor_params,
                         const double *h_acceptor_params, int32_t n_acceptors, int32_t n_acceptor_params) {
    HbondForce *hb = amm_force_get<HbondForce>(ctx, force_id, "amm_hbond_set_params");
    return hb ? amm_hbond_set_params_impl(ctx, hb, h_donor_params, n_donors, n_donor_params, h_acceptor_params, n_acceptors, n_acceptor_params) : 1;
}

int amm_hbond_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    HbondForce *hb = amm_force_get<HbondForce>(ctx, force_id, "amm_hbond_set_globals");
    return hb ? amm_hbond_set_globals_impl(ctx, hb, globals, nglobal) : 1;
}

int amm_hbond_stats(amm_ctx *ctx, int32_t force_id, int64_t *out) {
    HbondForce *hb = amm_force_get<HbondForce>(ctx, force_id, "amm_hbond_stats");
    if (!hb) return 1;
    if (!out) {
        amm_set_error("amm_hbond_stats: null argument");
        return 1;
    }
    return amm_hbond_stats_impl(ctx, hb, out);
}

int amm_hbond_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_HBOND, "amm_hbond_release"); }

// CustomManyParticleForce(3, any energy text) (csrc/manyparticle.hip): the compiled text and its variable table (atomsmm_amd/expr.py:
// compile_many_particle), the per-particle parameters, parameter-major, the dense type index of every particle and the permutation
// table over them, the excluded pairs of particles, the cutoff (rc <= 0: NoCutoff), whether displacements take the minimum image and
// the permutation mode (central != 0: UniqueCentralParticle)
int amm_many_create(amm_ctx *ctx, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst, const double *globals, int32_t nglobal,
                    const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars, int32_t n_particles, const double *h_params,
                    int32_t n_params, const int32_t *h_types, int32_t n_types, const int32_t *h_perm, const int32_t *h_excl, int32_t n_excl,
                    double rc, int32_t periodic, int32_t central, int32_t *force_id) {
    if (!ctx || !code || !force_id || (nconst > 0 && !consts) || (nglobal > 0 && !globals) || (n_vars > 0 && (!var_kinds || !var_slots)) ||
        (n_particles > 0 && !h_types) || !h_perm || (n_excl > 0 && !h_excl)) {
        amm_set_error("amm_many_create: null argument");
        return 1;
    }
    ManyForce *mf = nullptr;
    if (amm_many_create_impl(ctx, code, ncode, consts, nconst, globals, nglobal, var_kinds, var_slots, n_vars, n_particles, h_params, n_params,
                             h_types, n_types, h_perm, h_excl, n_excl, rc, periodic, central, &mf))
        return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_MANY_PARTICLE, mf);
    return 0;
}

int amm_many_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_particles, int32_t n_params, const int32_t *h_types,
                        int32_t n_types, const int32_t *h_perm) {
    ManyForce *mf = amm_force_get<ManyForce>(ctx, force_id, "amm_many_set_params");
    return mf ? amm_many_set_params_impl(ctx, mf, h_params, n_particles, n_params, h_types, n_types, h_perm) : 1;
}

int amm_many_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal) {
    ManyForce *mf = amm_force_get<ManyForce>(ctx, force_id, "amm_many_set_globals");
    return mf ? amm_many_set_globals_impl(ctx, mf, globals, nglobal) : 1;
}

int amm_many_stats(amm_ctx *ctx, int32_t force_id, int64_t *out) {
    ManyForce *mf = amm_force_get<ManyForce>(ctx, force_id, "amm_many_stats");
    if (!mf) return 1;
    if (!out) {
        amm_set_error("amm_many_stats: null argument");
        return 1;
    }
    return amm_many_stats_impl(ctx, mf, out);
}

int amm_many_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_MANY_PARTICLE, "amm_many_release"); }

// RMSDForce (csrc/rmsd.hip): the selected particles and the reference rows of those particles, in the list's order
int amm_rmsd_create(amm_ctx *ctx, const int32_t *h_particles, int32_t n_sel, const double *h_ref, int32_t *force_id) {
    if (!ctx || !force_id || (n_sel > 0 && (!h_particles || !h_ref))) {
        amm_set_error("amm_rmsd_create: null argument");
        return 1;
    }
    RmsdForce *rf = nullptr;
    if (amm_rmsd_create_impl(ctx, h_particles, n_sel, h_ref, &rf)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_RMSD, rf);
    return 0;
}

int amm_rmsd_set_reference(amm_ctx *ctx, int32_t force_id, const int32_t *h_particles, int32_t n_sel, const double *h_ref) {
    RmsdForce *rf = amm_force_get<RmsdForce>(ctx, force_id, "amm_rmsd_set_reference");
    if (!rf) return 1;
    if (n_sel > 0 && (!h_particles || !h_ref)) {
        amm_set_error("amm_rmsd_set_reference: null argument");
        return 1;
    }
    return amm_rmsd_set_reference_impl(ctx, rf, h_particles, n_sel, h_ref);
}

int amm_rmsd_stats(amm_ctx *ctx, int32_t force_id, int64_t *out) {
    RmsdForce *rf = amm_force_get<RmsdForce>(ctx, force_id, "amm_rmsd_stats");
    if (!rf) return 1;
    if (!out) {
        amm_set_error("amm_rmsd_stats: null argument");
        return 1;
    }
    return amm_rmsd_stats_impl(rf, out);
}

int amm_rmsd_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_RMSD, "amm_rmsd_release"); }

// GayBerneForce (csrc/gayberne.hip): the interacting particles compacted by the caller, their exceptions as a CSR over the compacted
// indices and the reverse table of the axis particles
int amm_gayberne_create(amm_ctx *ctx, const int32_t *h_active, int32_t n_active, const int32_t *h_axes, const double *h_par, const int32_t *h_ex_ptr,
                        const int32_t *h_ex_col, const double *h_ex_par, const int32_t *h_rev_ptr, const int32_t *h_rev_src, double cutoff,
                        double switch_distance, int32_t periodic, int32_t *force_id) {
    if (!ctx || !force_id || !h_rev_ptr || (n_active > 0 && (!h_active || !h_axes || !h_par || !h_ex_ptr))) {
        amm_set_error("amm_gayberne_create: null argument");
        return 1;
    }
    if (n_active > 0 && h_ex_ptr[n_active] > 0 && (!h_ex_col || !h_ex_par)) {
        amm_set_error("amm_gayberne_create: null argument");
        return 1;
    }
    if (h_rev_ptr[ctx->n] > 0 && !h_rev_src) {
        amm_set_error("amm_gayberne_create: null argument");
        return 1;
    }
    GayBerneForce *gf = nullptr;
    if (amm_gayberne_create_impl(ctx, h_active, n_active, h_axes, h_par, h_ex_ptr, h_ex_col, h_ex_par, h_rev_ptr, h_rev_src, cutoff, switch_distance,
                                 periodic, &gf))
        return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_GAYBERNE, gf);
    return 0;
}

int amm_gayberne_set_params(amm_ctx *ctx, int32_t force_id, const double *h_par, int32_t n_active, const double *h_ex_par, int32_t n_entries) {
    GayBerneForce *gf = amm_force_get<GayBerneForce>(ctx, force_id, "amm_gayberne_set_params");
    if (!gf) return 1;
    return amm_gayberne_set_params_impl(ctx, gf, h_par, n_active, h_ex_par, n_entries);
}

int amm_gayberne_stats(amm_ctx *ctx, int32_t force_id, int64_t *out) {
    GayBerneForce *gf = amm_force_get<GayBerneForce>(ctx, force_id, "amm_gayberne_stats");
    if (!gf) return 1;
    if (!out) {
        amm_set_error("amm_gayberne_stats: null argument");
        return 1;
    }
    return amm_gayberne_stats_impl(ctx, gf, out);
}

int amm_gayberne_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_GAYBERNE, "amm_gayberne_release"); }

// DrudeForce (csrc/drude.hip): the rows of the object model; the library derives the spring constants and the pair parameters
int amm_drude_create(amm_ctx *ctx, const int32_t *h_idx, const double *h_par, int32_t n_drude, const int32_t *h_pair, const double *h_thole,
                     int32_t n_pairs, int32_t periodic, int32_t *force_id) {
    if (!ctx || !force_id || (n_drude > 0 && (!h_idx || !h_par)) || (n_pairs > 0 && (!h_pair || !h_thole))) {
        amm_set_error("amm_drude_create: null argument");
        return 1;
    }
    DrudeForce *df = nullptr;
    if (amm_drude_create_impl(ctx, h_idx, h_par, n_drude, h_pair, h_thole, n_pairs, periodic, &df)) return 1;
    *force_id = amm_force_register(ctx, AMM_FORCE_DRUDE, df);
    return 0;
}

int amm_drude_set_params(amm_ctx *ctx, int32_t force_id, const int32_t *h_idx, const double *h_par, int32_t n_drude, const int32_t *h_pair,
                         const double *h_thole, int32_t n_pairs) {
    DrudeForce *df = amm_force_get<DrudeForce>(ctx, force_id, "amm_drude_set_params");
    if (!df) return 1;
    return amm_drude_set_params_impl(ctx, df, h_idx, h_par, n_drude, h_pair, h_thole, n_pairs);
}

int amm_drude_release(amm_ctx *ctx, int32_t force_id) { return amm_force_release(ctx, force_id, AMM_FORCE_DRUDE, "amm_drude_release"); }

}   // extern "C"
