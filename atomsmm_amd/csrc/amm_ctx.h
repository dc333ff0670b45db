// atomsmm_amd/csrc/amm_ctx.h -- internal structures of libatomsmm_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/atomsmm_hip.h"

#define AMM_WAVE 64
#define AMM_MAX_PRE 6            // kicks that can ride on one inner-loop launch
#define AMM_DERIV_LAMBDA 1024   // internal PairConsts flag: energy output = dE/dlambda (softcore family)
#define AMM_MAX_GROUPS 33   // 0..31 = OpenMM force groups, 32 = all forces (`f`)

void amm_set_error(const std::string &msg);
#define AMM_HIP(call)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            amm_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                    \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)
// a device array of its own for `count` host values (one element when there are none: the pointer is never null)
template <typename T>
inline int amm_upload(T **dst, const T *src, size_t count) {
    AMM_HIP(hipMalloc(dst, sizeof(T) * (count ? count : 1)));
    if (count) AMM_HIP(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return 0;
}

// Radial Coulomb table of a pair force (pair_tab.h): abscissa w = r^2 * scale, interval = (hi32(w) >> 13) - base.
struct PairTab {
    double scale, r2min;                // r2 < r2min: below the table (analytic path)
    int baseA, nA;                      // zone A (w < 1): interval = (hi32(w) >> 13) - baseA, nA intervals
    int shiftB, rawB_minus_nA, halfB;   // zone B (w >= 1): interval = (hi32(w) >> shiftB) - rawB_minus_nA
    int nint;                           // all intervals; 0: the family has no table
    int ss_first;                       // site-site table (pair_tab.h): first interval it covers; -1: none
    double ss_r2min;                    // site pairs closer than this are below it (analytic path)
};

// Constants of one pair force, precomputed on the host and passed to kernels by value.
struct PairConsts {
    int family, flags, degree, cmode;   // cmode: 0 plain coulomb, 1 ewald(erfc), 2 reaction field
    double sign, rc2, rc0, rs0, inv_dr0, rswitch, rc;
    double alpha, two_alpha_over_sqrtpi, Kc, krf, crf;
    double inv_rc0, inv_rc0_2;          // shift / force-switch constants
    double b, f12c, f6c, f1c;           // force-switch (forces.py:559-563)
    double sw_den, inv_sw_dr;           // DAMPED: rc^d - rs^d ; NONBONDED: 1/(rc - rswitch)
    double inv_sw_den, rswitch_d;       // DAMPED: 1/(rc^d - rs^d), rs^d
    PairTab tab;
};

struct Box {
    double L[3], invL[3];
};

// force rows to clear (hybrid lists: the atoms outside the molecules), served by the molecule-row chain's sort / gather launch
struct CZeroRows {
    int n;
    const int *idx;
    double *f0, *f1;
};

struct CellGrid {
    int nc[3];
    int nstencil[3];   // number of unique neighbour cells visited per axis (2h+1, or all nc cells)
    int h[3];          // stencil half-width in cells
    int ncell;
    double cw[3], inv_cw[3];
};

struct ClusterList;   // cluster.h: molecule-row list of the force-only traversal
struct SmallGroup;    // group.hip: interaction-group force with one small set, evaluated without a neighbour list
struct PairExpr;      // pair_expr_vm.h: compiled energy text of a generic pair force (AMM_PAIR_EXPR)
struct PairArgs;      // pair_args.h: launch arguments of the per-atom-row traversals

struct PairForce {
    amm_pair_desc desc;
    bool free_space = false;       // AMM_FREE_SPACE: all pairs at the distance the positions give (free.hip) -- no grid, no list, no rebuild
    ClusterList *cl = nullptr;     // molecule rows (built on the first force-only evaluation of a qualifying force; list owners only)
    bool cluster_ok = false;       // the force has three-site molecules (their three pairs their only exclusions) and walks molecule rows
    // Hybrid list: molecule rows for the pairs of two such molecules + per-atom rows, kept by a hidden child force (`rest`, filtered to
    // the pairs that involve an atom outside the molecules), for everything else -- an ion, a solute, a chain next to the waters.
    bool hybrid = false;
    PairExpr *expr = nullptr;      // AMM_PAIR_EXPR: the program k_pair_expr interprets (pair_expr.hip); the three parameter arrays hold RAW values
    SmallGroup *small = nullptr;   // interaction-group force whose smaller set has <= 128 atoms (group.hip): no list at all
    std::vector<int> h_excl_ptr, h_excl_idx;    // host copy of the exclusion CSR (interaction-group forces)
    PairForce *rest = nullptr;     // the child (registered in ctx->forces behind its parent, in no group)
    bool hybrid_rest = false;      // this force IS such a child: its list keeps the pairs with at least one rest atom (code 2)
    int profile_id = -1;           // a child is timed when its parent is (amm_profile_enable with a force id): the parent's id
    std::vector<int> h_mol_first;  // first atom of every molecule; empty: molecule m = atoms 3 m .. 3 m + 2 (no rest atoms)
    int n_mol = 0, n_rest = 0;
    int *d_mol_first = nullptr, *d_rest_idx = nullptr;
    bool force_rebuild_c = false;  // the molecule rows carry site bits of another site pattern
    bool one_site_class = false;   // all atoms with eps != 0 share ONE (sigma, eps): the molecule-row kernels carry them as constants
    double site_hsig = 0, site_seps2 = 0;
    bool site_one_charge = false;  // ... and ONE charge (site_q): the site-site radial table of pair_tab.h can stand for their pairs
    double site_q = 0;
    int site_atoms = 7;            // bit a set when atom 3 m + a of some molecule m has a site (molecule-row forces)
    double *d_tab_ss = nullptr;    // site-site table [nint - ss_first][6] (molecule-row kernels); null: none
    double ss_error = 0;           // its largest relative interpolation error
    double ss_built_for[3] = {0, 0, 0};     // (sigma/2, 2 sqrt(eps), q) the tables were last built for
    const double *d_lambda_dev = nullptr;      // softcore family: lambda is read from this device scalar at launch time (amm_pair_set_lambda_dev)
    bool all_q_zero = false;       // every charge is zero (set_params): the per-atom-row kernel has an instantiation without the Coulomb table
    int last_chargeless = 0;       // ... and the last force-only evaluation ran it (statistics)
    int last_fused = 0;            // 1: the last force-only evaluation rode on the list owner's launch (molecule rows, fused pass)
    double last_gfac = 0;          // ... then: this force's factor relative to the host, (Kc sign)_guest / (Kc sign)_host, and
    int last_gunit = 0;            // whether the launch took the kernel that leaves the product by it out (gfac == 1.0; statistics)
    int last_kind = 0;             // list walked by the last evaluation: 0 per-atom rows, 1 molecule rows, 2 hybrid (statistics)
    PairConsts pc;
    int n = 0;
    int id = -1;                   // force id within the context
    double skin = 0, rlist = 0;
    double skin_out_req = -1;      // the context's outer buffer when the force was created (<= 0: none asked for)
    double skin_req = 0;           // the buffer asked for at creation, before the box clamps it: amm_set_box derives `skin` from it again
    double built_L[3] = {0, 0, 0}; // box edges at the first build of the per-atom rows, and rlist_build^3 / V then: the row capacity was
    double built_rows = 0;         // sized for that density (amm_set_box trusts it while this quantity has grown by less than a quarter)
    int ncell_alloc = 0;           // cells the per-cell arrays below were allocated for
    double rlist_build = 0;        // rlist + fp32 safety margin used by the prune pass (inner list)
    double skin_out = 0;           // outer Verlet buffer (cell-built list, radius rc + skin_out)
    double rlist_out_build = 0;
    // per-atom parameters, original order: q, sigma/2, 2*sqrt(eps)
    double *d_q = nullptr, *d_hsig = nullptr, *d_seps2 = nullptr;
    int *d_excl_ptr = nullptr, *d_excl_idx = nullptr;
    CellGrid grid;
    int *d_cell_of = nullptr, *d_cell_count = nullptr, *d_cell_start = nullptr;
    int *d_cell_members = nullptr;   // [ncell][capc] atoms of each cell in arrival order (k_cell_assign)
    int capc = 0;
    int *d_perm = nullptr, *d_inv_perm = nullptr;
    double4 *d_posq_s = nullptr;   // sorted: wrapped x,y,z and charge
    double2 *d_lj_s = nullptr;     // sorted: sigma/2, 2*sqrt(eps)
    // per-atom rows: sorted copies written ahead of time by the launch that moved the atoms (pair.hip: the kernel's epilogue)
    PairForce *a_sorted_for = nullptr;
    long a_sorted_epoch = -1;
    const double *a_sorted_pos = nullptr;
    double4 *d_posq_alt = nullptr; // molecule rows: second copy of d_posq_s, for an epilogue that writes the sorted positions of the NEXT evaluation of this same force
    float4 *d_pos4f_s = nullptr;   // sorted fp32 positions at the last list build
    double *d_xref = nullptr;      // positions at the last prune (original order)
    double *d_xref_out = nullptr;  // positions at the last outer (cell-based) build
    int s_begin = 0, s_end = 0;    // sorted-slot range owned by this rank
    int cap = 0;
    int *d_nl = nullptr, *d_nnb = nullptr, *d_nnb_near = nullptr;   // inner list (traversed)
    int *d_nl_out = nullptr, *d_nnb_out = nullptr, *d_nnb_scratch = nullptr;   // outer list (pruned from)
    int cap_out = 0;
    bool dual = false;             // outer list + prune (skin_out > skin) or a single list built from the cells
    PairForce *host = nullptr;     // owner of the neighbour list this force traverses (nullptr: its own)
    int fuse_ok = -1;              // cached amm_pair_can_fuse_discount(this, host) (reset by set_params)
    int dual_ok = -1;              // cached amm_pair_can_eval_dual(this, host): -1 unknown, 0 no, 1 yes (reset by set_params)
    double rnear_build = 0;        // list radius of the guest force sharing this list (front part of each row)
    int *d_flags = nullptr;        // [0] need prune [1] overflow [2] max inner row [4] need outer build [5] max outer row
    unsigned long long *d_counters = nullptr;  // [0] prunes [1] inner pairs [2] inner front pairs [3] outer pairs [4] outer builds
    unsigned long long *d_blockstats = nullptr; // per build-kernel block: (sum, max) of list lengths
    int *d_ticket = nullptr;       // last-block tickets: [0] cell assign/scan [1] list build/statistics
    long checked_epoch = -1;       // ctx->pos_epoch / position buffer of the last displacement check
    const double *checked_pos = nullptr;
    long pre_epoch = -1;           // same, for a check already made by the kernel that moved the atoms
    const double *pre_pos = nullptr;
    int lpa = 8;                   // lanes per i-atom in the traversal kernel
    int parts = 1;                 // wavefronts per cell in the list-build kernel
    double *d_epart = nullptr;
    int n_epart = 0;
    double *d_tab = nullptr;       // radial Coulomb table: pc.tab.nint x 6 doubles (pair_tab.h)
    unsigned long long tab_serial = 0;     // of this upload of d_tab / d_tab_ss (amm_pair_build_table): no two uploads share one
    // what the molecule-row kernels stage when this force's Coulomb table comes first in LDS (cluster.hip: cpair_tab_image): the
    // launch's tables in one array, by what it holds (bit 0: a guest's tables too, bit 1: site-site tables); made of the uploads
    // with these serial numbers by copies on `stream`
    struct TabImage {
        char *d = nullptr;
        size_t bytes = 0;
        unsigned long long host_serial = 0, guest_serial = 0;
        hipStream_t stream = nullptr;
    } tab_image[4];
    double tab_error = 0;          // largest relative interpolation error found when the table was built
    int *d_cls = nullptr;          // per atom (original order): 1 = no Lennard-Jones site (eps = 0) -- sorted behind the others in its cell
    int *d_cell_count_lj = nullptr, *d_cell_start_lj = nullptr;   // per cell: atoms WITH a Lennard-Jones site (count, exclusive scan)
    std::vector<int> h_cls;        // host copy of d_cls: a change of the site pattern (parameter offsets on epsilon) asks for a rebuild
    bool force_rebuild = false;    // the rows' site counts and traversal order were made for another site pattern
    int sites_match = -1;          // a guest may use its list owner's site counts only if both have sites on the same atoms (-1: unknown)
    int *d_nnb_lj = nullptr;       // per row: how many of its entries are partners with a Lennard-Jones site (front | back << 16): they come first on either side
    int *d_cell_sets = nullptr;    // interaction-group forces: per cell, which of the two sets have atoms in it (bit 0 / bit 1)
    int active_cap = 0;            // rows the pair kernels' grid covers when d_active is walked
    int active_size = 0;           // slots of d_active (long rows are filed from its front, short ones from its back)
    int *d_active = nullptr;       // filtered lists: slice-relative rows that hold entries (their number: flags[8])
    float *d_member = nullptr;     // interaction-group forces: set code of each atom (0 none, 1, 2); the list keeps only (1, 2) pairs
    int *d_row_order = nullptr;    // traversal order of the slice's rows: rows with a Lennard-Jones site first (wave-uniform LJ skip)
    bool built = false;
    int64_t n_evals = 0;
    // profiling
    std::vector<hipEvent_t> ev;    // pairs (start, stop)
    size_t ev_used = 0;
};

#ifndef AMM_TICKET_INTS
#define AMM_TICKET_INTS 64      // ints per last-block ticket (device_utils.h: amm_last_block)
#endif

struct BondedSet {
    // host staging
    std::vector<int32_t> h_idx[8];
    std::vector<double> h_par[8];
    int periodic[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool has_near = false;
    amm_pair_desc near_desc;
    PairConsts near_pc;
    double ewald_alpha = 0, ewald_Kc = 0;
    double ljc_Kc = 138.935456;
    bool sliced = false;           // world > 1: compute only this rank's rows (group is all-reduced by the host)
    bool finalized = false;
    // device: CSR per atom of packed (atom, term) records
    int n_terms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int *d_ref_ptr = nullptr;      // [n+1]
    int4 *d_rec_a = nullptr;       // atoms of the term
    double4 *d_rec_q = nullptr;    // parameters + kind/role/periodic code
    int4 *d_rec_l = nullptr;       // atoms of the term as slots within their connected component
    int *d_comp_ptr = nullptr, *d_comp_atoms = nullptr;   // connected components of the term graph (CSR)
    int ncomp = 0, max_comp = 0;
    int G = 4;                     // lanes per component: what the term tables are sized by and the inner-components launch runs with
    // term-parallel inner loop: every component has at most G terms (G lanes per component) -> lane l evaluates term l
    bool terms_ok = false;
    // ... and, further, every component is one three-site molecule {3 c, 3 c + 1, 3 c + 2} (slot = atom order) with at most four terms,
    // all of them harmonic bonds / angles (a box of flexible three-site water): the row owner of a molecule-row pair kernel can then
    // run the inner RESPA loop of its molecules as the kernel's epilogue (cluster.hip: cepi_rows)
    bool mol3_ok = false;
    int4 *d_term_l = nullptr;                 // [ncomp*G] atoms of the term as component slots (x < 0: no term)
    double4 *d_term_q = nullptr;              // [ncomp*G] parameters + kind/periodic code
    unsigned long long *d_atom_recs = nullptr; // [n] the atom's records as (term slot | role << 3) in 5-bit fields, count in bits 60..63
    // term-parallel evaluation of large sets (force only): every term once, its per-role forces parked in d_tf, every atom
    // then adds up its records from there in record order -- the numbers and the order of k_bonded
    int n_gterms = 0;
    int4 *d_gt_a = nullptr;        // [n_gterms] atoms of the term
    double4 *d_gt_q = nullptr;     // [n_gterms] parameters + kind/periodic code
    int *d_rec_src = nullptr;      // [nref] term * 4 + role of each (atom, term) record
    double *d_tf = nullptr;        // [n_gterms][4][3]
    // mixed sets (waters + a chain: config C5) on the fused EVAL + kicks path: the SMALL components (<= 4 atoms, <= 4 terms: a water)
    // are evaluated four lanes per component from registers / LDS (no parked forces, no gather); only the atoms and terms of the big
    // components go through the term-parallel arrays above
    bool mixed_ok = false;
    int n_sc = 0;                                   // small components
    int4 *d_sc_atoms = nullptr;                     // [n_sc] their atoms (-1 padded)
    int4 *d_sc_term_l = nullptr;                    // [n_sc*4] atoms of the component's terms as slots 0..3 (x < 0: no term)
    double4 *d_sc_term_q = nullptr;                 // [n_sc*4]
    unsigned long long *d_sc_recs = nullptr;        // [n_sc*4] per (component, atom slot): the atom's records, as d_atom_recs
    int n_big = 0, n_bigterms = 0;
    int *d_big_atoms = nullptr;                     // atoms of the other components
    int *d_big_terms = nullptr;                     // global indices of their terms (into d_gt_a / d_gt_q / d_tf)
    double *d_epart = nullptr;
    int n_epart = 0;
};

struct PmeForce;      // pme.hip
struct ConstraintSet; // constraints.hip
struct MinObj;        // minimize.hip: one L-BFGS minimisation (history ring, Gram matrix, direction)
struct TermExprForce; // term_expr_vm.h: bond / angle / torsion / external terms with a compiled energy text (term_expr.hip)

struct CvForce;       // cv.hip: a CustomCVForce -- K inner forces and the compiled outer text over their energies
struct CompoundForce; // compound.hip: a CustomCompoundBondForce / CustomCentroidBondForce -- bonds over several particles or centres
struct GbForce;       // gb.hip: a GBSAOBCForce -- generalized-Born (OBC2) implicit solvent with a surface-area term, free space only
struct CmapForce;     // cmap.hip: a CMAPTorsionForce -- bicubic maps over pairs of dihedrals
struct CustomGbForce; // custom_gb.hip: a CustomGBForce -- computed per-particle values and energy terms written as text, free space only
struct HbondForce;    // hbond.hip: a CustomHbondForce -- donors against acceptors over all pairs, the energy written as text
struct ManyForce;     // manyparticle.hip: a CustomManyParticleForce -- sets of three particles under a cutoff, the energy written as text
struct RmsdForce;     // rmsd.hip: an RMSDForce -- the deviation of selected particles from a reference after the best rigid fit
struct GayBerneForce; // gayberne.hip: a GayBerneForce -- ellipsoids whose frames other particles define, over all pairs of interacting particles
struct DrudeForce;    // drude.hip: a DrudeForce -- anisotropic springs between Drude particles and their parents, Thole-screened dipole pairs
// The force families.  A family is described ONCE: its tag here, the struct that goes with the tag in amm_force_type, and its row of
// the table behind amm_family (families.hip).  The typed lookup and its refusals, amm_force_eval_dispatch, release, amm_destroy, amm_set_slice and
// cv.hip's messages all read the row -- a new family adds these three lines, its own .hip file and its extern "C" entry points.
// Fourteen families today (and the tag of a released id).
enum : int { AMM_FORCE_RELEASED = 0, AMM_FORCE_PAIR = 1, AMM_FORCE_BONDED = 2, AMM_FORCE_PME = 3, AMM_FORCE_TERM_EXPR = 4, AMM_FORCE_CV = 5,
             AMM_FORCE_COMPOUND = 6, AMM_FORCE_GB = 7, AMM_FORCE_CMAP = 8, AMM_FORCE_CUSTOM_GB = 9, AMM_FORCE_HBOND = 10,
             AMM_FORCE_MANY_PARTICLE = 11, AMM_FORCE_RMSD = 12, AMM_FORCE_GAYBERNE = 13, AMM_FORCE_DRUDE = 14,
             AMM_FORCE_TYPES = 15 };   // ForceObj::type, the row amm_family returns
template <class T> inline constexpr int amm_force_type = -1;
template <> inline constexpr int amm_force_type<PairForce> = AMM_FORCE_PAIR;
template <> inline constexpr int amm_force_type<BondedSet> = AMM_FORCE_BONDED;
template <> inline constexpr int amm_force_type<PmeForce> = AMM_FORCE_PME;
template <> inline constexpr int amm_force_type<TermExprForce> = AMM_FORCE_TERM_EXPR;
template <> inline constexpr int amm_force_type<CvForce> = AMM_FORCE_CV;
template <> inline constexpr int amm_force_type<CompoundForce> = AMM_FORCE_COMPOUND;
template <> inline constexpr int amm_force_type<GbForce> = AMM_FORCE_GB;
template <> inline constexpr int amm_force_type<CmapForce> = AMM_FORCE_CMAP;
template <> inline constexpr int amm_force_type<CustomGbForce> = AMM_FORCE_CUSTOM_GB;
template <> inline constexpr int amm_force_type<HbondForce> = AMM_FORCE_HBOND;
template <> inline constexpr int amm_force_type<ManyForce> = AMM_FORCE_MANY_PARTICLE;
template <> inline constexpr int amm_force_type<RmsdForce> = AMM_FORCE_RMSD;
template <> inline constexpr int amm_force_type<GayBerneForce> = AMM_FORCE_GAYBERNE;
template <> inline constexpr int amm_force_type<DrudeForce> = AMM_FORCE_DRUDE;
struct ForceFamily {
    const char *noun, *tag, *prefix;   // "a CMAP force", "AMM_FORCE_CMAP", "amm_cmap_*"
    const char *bad_id;                // what the family's entry points say of an id that is not theirs (behind "<entry point>: " if they name themselves)
    bool single_rank;                  // amm_set_slice refuses world > 1 while such a force lives
    int (*eval)(amm_ctx *ctx, void *obj, const double *d_pos, double *d_force, int accumulate, double *d_energy);
    void (*free)(void *obj);           // the device memory AND the object
};
const ForceFamily &amm_family(int type);   // the row of AMM_FORCE_<type>
// one object of the family `type` says; a released id holds none
struct ForceObj {
    int type = AMM_FORCE_RELEASED;
    void *obj = nullptr;
    template <class T> T *as() const { return type == amm_force_type<T> ? static_cast<T *>(obj) : nullptr; }    // null: another family's
    PairForce *pair() const { return as<PairForce>(); }
    BondedSet *bonded() const { return as<BondedSet>(); }
};

struct ExprDef {
    std::vector<int32_t> code;
    std::vector<double> consts, globals;
};

// native bath step of Langevin-type integrators: v <- z v + sqrt(kT (1 - z^2) / m) * gaussian  (propagators.py:727-741)
// kind 1 (Nose-Hoover-Langevin, NHL_R_Integrator: propagators.py:1362-1449 as MassiveNoseHooverLangevin emits it): the
// three per-DOF steps  v <- v exp(-h w) ; w <- z w + sqrt(kT (1 - z^2)/Q) gaussian + (m v^2 - kT)(1 - z)/(Q friction) ;
// v <- v exp(-h w)  with the thermostat velocity w of each DOF in the per-DOF buffer `slot`.
// kind 2 (stochastic-isokinetic, SIN_R_Integrator with L = 1: propagators.py:276-355, 1045-1105): v1 <- v1 exp(-h v2) ;
// isokinetic rescale of (v, v1) ; v2 <- z v2 + sqrt(kT (1 - z^2)/Q2) gaussian + (Q1 v1^2 - kT)(1 - z)/(Q2 friction) ;
// v1 <- v1 exp(-h v2) ; rescale -- thermostat velocities v1 in the context's isokinetic slot, v2 in `slot`.
// kinds 3..6 (regulated Nose-Hoover-Langevin, propagators.py:1598-2007): 3 massive, 4 twice-regulated massive, 5 atomic, 6
// twice-regulated atomic -- [boost of w ;] scaling of v ; Ornstein-Uhlenbeck step of w ; scaling of v [; boost of w] (`split`: the
// boosts are there and the OU step has no drift), w in `slot`; the atomic kinds keep one w per atom in all three components.
// amm_reg_bath_step (expr_vm.h) has the arithmetic.
struct BathDef {
    double z, kT;
    int kind = 0;                  // 0 Ornstein-Uhlenbeck, 1 Nose-Hoover-Langevin, 2 stochastic-isokinetic, 3..6 regulated
    double h = 0, Q = 0, friction = 0;
    int slot = -1;
    int split = 0;                 // regulated kinds: boosts of w around the block, OU step without drift
    double omega = 0, alpha = 1, an = 1;   // regulated kinds: noise amplitude, alpha_n, alpha_n n
    double kfac = 1;               // twice-regulated kinds: (n + 1)/(alpha_n n), the factor of m v^2 in the drive
};

// One of OpenMM's stock integrators (amm_stock_define; stock.hip): a = exp(-friction dt), b = (1 - a)/friction (dt when friction = 0)
struct StockDef {
    int kind = 0;                  // AMM_STOCK_*
    double dt = 0, friction = 0, kT = 0, a = 1, b = 0;
};

// The step of a DrudeLangevinIntegrator (amm_drude_step_define; drude.hip): a, b as in StockDef from the friction of the ordinary atoms
// and of the centres of mass, aD, bD from the friction of the relative motion of a pair; wall: the hard wall distance, 0: none
struct DrudeStepDef {
    double dt = 0, kT = 0, kTD = 0, a = 1, b = 0, aD = 1, bD = 0, wall = 0;
    int n_pairs = 0;
    int *d_drude_of = nullptr;     // [n] the Drude particle an atom is the parent of, -1: none
    int *d_parent_of = nullptr;    // [n] the parent of a Drude particle, -1: not a Drude particle
    int *d_flag = nullptr;         // set when a pair is beyond twice the hard wall (amm_check reads and clears it)
};

// Regulated mode of a context (RegulatedTranslationPropagator, propagators.py:1537-1575): every AMM_OP_MOVE is
//   x <- x + c tanh(alpha v / c) coef,  c = sqrt(an_kT / m)
// (amm_reg_dx, expr_vm.h), so that no degree of freedom moves faster than c.
struct RegDef {
    bool on = false;
    double alpha = 1, an_kT = 0;
};

// Isokinetic mode of a context (SIN(R), L = 1): every AMM_OP_KICK is the isokinetic kick
//   v <- v cosh(z) + sqrt(LkT/m) sinh(z), z = coef F / sqrt(m LkT) ;  H = sqrt(LkT / (m v^2 + Q1 v1^2 / 2)) ; v <- H v ; v1 <- H v1
// with the per-DOF thermostat velocity v1 in buffer `slot` (MassiveIsokineticPropagator, propagators.py:276-355).
struct IsoDef {
    bool on = false;
    double LkT = 0, Q1 = 0;
    int slot = -1;
};

struct GroupDef {
    int slot = -1;
    std::vector<int> forces;
    int exchange = 0;              // AMM_EXCHANGE_*: how the forces of the rank's slice reach the other ranks
};

// exchange of owner-computed force slices: the pair kernel leaves the rows of this rank's slice of the
// cell-sorted order in chunk `rank` of the exchange buffer, the chunks are all-gathered, and k_unsort spreads the
// gathered rows to the group's buffer in atom order (every rank holds the same permutation).
struct PendingExchange {
    bool active = false;
    int per = 0, nf = 0;           // slots per rank; forces per chunk (2 after a dual evaluation)
    const int *perm = nullptr;
    double *force = nullptr, *gforce = nullptr;
    // kind 1: the chunks hold the STATE of the ranks' molecules -- [x: per x 3][v: per x 3] in cell-sorted order -- after an
    // evaluation whose launch integrated them (cluster.hip: cepi_rows on a rank's slice); finishing it spreads the other ranks'
    // positions and velocities to the atom-order arrays, evaluates the lists' displacement triggers for them and writes the next
    // evaluation's sorted copies of their molecules (k_state_scatter)
    int kind = 0;
    ClusterList *cl = nullptr;
    PairForce *next = nullptr;     // the force whose sorted copies the next pair evaluation reads (or none)
};

// a neighbour list whose displacement trigger the kernel that moves the atoms evaluates (saves the check launch)
#define AMM_MAX_WATCH 4
struct ListWatch {
    const double *xref = nullptr;
    double thr2 = 0;
    int *flags = nullptr;
    long *pre_epoch = nullptr;
    const double **pre_pos = nullptr;
};

// slots per rank of the cell-sorted order: whole molecules of three (the molecule rows slice by molecule)
static inline int amm_slice_per(int n, int world) {
    const int nc = (n + 2) / 3;
    return 3 * ((nc + world - 1) / world);
}

// What follows a force-only pair evaluation in the step program when it is `[KICK ...] ; n x { KICK(f0) ; MOVE ; EVAL(group of f0) ; KICK(f0) }`
// with the innermost group one bond-list set of three-site molecules (BondedSet::mol3_ok): amm_run_ops hands it to the evaluation, and a
// molecule-row kernel runs it as its epilogue -- the wavefront that has just summed a molecule's rows kicks, moves and re-evaluates that
// molecule (no other atom enters) and writes the sorted copies of the next pair evaluation (cluster.hip: cepi_rows).
struct EpiPlan {
    BondedSet *bs = nullptr;
    double *f0 = nullptr;              // the innermost group's force buffer
    int npre = 0, niter = 0;
    const double *pre_a[AMM_MAX_PRE] = {nullptr}, *pre_b[AMM_MAX_PRE] = {nullptr};
    double pre_coef[AMM_MAX_PRE] = {0};
    int pre_plus[AMM_MAX_PRE] = {0};
    double c1 = 0, d = 0, c2 = 0;
    PairForce *next = nullptr;         // the force whose sorted copies the next pair evaluation reads (nullptr: not known)
    // kind 1: per-atom rows (pair.hip, AtomEpiArgs) -- the ops behind the EVAL are plain kicks and, maybe, a move (velocity Verlet):
    // the kicks are pre_*[0 .. npre), niter = 0
    int kind = 0;
    int with_move = 0;
    double dcoef = 0;
};

struct amm_ctx {
    int n = 0;
    int opt_spec_assign = 1;           // ... which also files the moved molecules in their cells ahead of a possible rebuild (no assign launch)
    int opt_state_exchange = 1;        // multi-rank: launches that integrate their rows' molecules exchange positions and velocities, not forces
    int opt_chargeless = 1;            // per-atom rows: the chargeless instantiation of the tabulated kernel for forces whose charges are all zero
    int opt_fuse_epilogue = 1;         // molecule rows: the inner RESPA loop of a box of three-site molecules as the pair kernel's epilogue
    const EpiPlan *epi_request = nullptr;   // amm_run_ops -> amm_cluster_eval_impl (one evaluation)
    bool epi_done = false;             // ... which says here whether its launch carried the plan (it then bumped pos_epoch itself)
    long long n_epilogues = 0;         // launches that did (statistics)
    long long n_state_exchanges = 0;   // ... on a rank's slice, followed by an exchange of positions and velocities instead of forces
    // force buffers that hold THIS RANK'S rows only (written by such launches: the kicks they feed ran on this rank's molecules,
    // nobody else needs them) until their group is evaluated again in full: amm_run_ops refuses -- or, for bond-list groups,
    // re-evaluates -- before an op reads one for all atoms
    std::vector<const double *> own_only;
    long long n_sched = 0;             // scheduling decisions of amm_run_ops so far: launches of the step program, an evaluation counted as one
    long long n_copies_current = 0;    // evaluations that found their sorted copies in place (no gather launch)
    long long n_rule[7] = {0};         // ... per taker: [0] the plain path, [1..6] the fusion rules in run_ops.hip's numbering (their sum is n_sched)
    long long n_plan_offers = 0;       // evaluations that amm_run_ops offered an epilogue plan (carried or not: n_epilogues counts the carried)
    // tuning / test options (amm_set_option): never read from the environment, so that a stray variable cannot change the
    // order of summation of a production run
    int opt_cluster = 1;           // molecule rows for qualifying forces (0: per-atom rows everywhere)
    int opt_hybrid = 1;            // ... also when the three-site molecules share the box with other atoms (hybrid lists)
    double opt_rest_skin_factor = 2.0;   // Verlet buffer of a hybrid list's per-atom part relative to its molecule rows
    int opt_mixed_terms = 1;       // mixed bond-list sets: small components four lanes each on the fused EVAL + kicks path (bonded.hip)
    int opt_small_group = 1;       // interaction-group forces with a small set (a solute) without a neighbour list (group.hip)
    bool creating_rest = false;    // amm_pair_create is making the hidden child of a hybrid list
    int opt_tab = 1;               // tabulated force-only kernels (0: the analytic kernels)
    int opt_build_split = 0;       // split-stream list build (k_cbuild_split): 0 = off, -1 = for slices (world > 1) with the library's choice of blocks per cell, k > 0 = k blocks per cell
    int opt_lpa = 0, opt_parts = 0, opt_unroll = 2, opt_dual_unroll = 2, opt_tab_bs = 0, opt_tab_dual_bs = 0;
    int opt_site_tab = 1;               // molecule rows: site-site radial tables instead of Lennard-Jones arithmetic where a force has one
    CZeroRows zero_rows = CZeroRows{0, nullptr, nullptr, nullptr};      // pending request (pair.hip -> cluster.hip, one evaluation)
    int opt_positions_private = 0;      // amm_run_ops does not assume the caller moved the atoms between calls (amm_positions_changed says so)
    int opt_group_candidates = 1;       // list-free group forces on the fused inner loop: walk the atoms near the small set only while a companion list vouches for them
    int opt_row_phases = 1;             // molecule rows: the remainder of the rows after whole rounds of tasks goes out in smaller tasks (cpair_plan)
    int opt_fuse_rows = 1;              // molecule rows: host + guest force of a shared list in ONE launch when a fused kernel exists
    int opt_terms_from = 8192, opt_no_term_lanes = 0;
    int opt_gb_lpr = 0;                 // lanes per row of the generalized-Born passes (gb.hip): 0 = amm_free_lanes_per_row(n); 1, 2, 4 .. 64
    int opt_cgb_lpr = 0;                // ... and of the custom generalized-Born passes (custom_gb.hip)
    int opt_hbond_chunks = 0;           // column chunks per row of a hydrogen-bond force created from now on (hbond.hip): 0 = chosen from the row count
    int opt_hbond_compact = 1;          // ... and whether its survivors queue up for the interpreter (0: drained batch by batch -- a measurement)
    int opt_many_capacity = 256;        // neighbours a row of a many-particle force with a cutoff created from now on can hold (manyparticle.hip): a multiple of 64
    int opt_rmsd_blocks = 0;            // blocks of an RMSD force created from now on (rmsd.hip): 0 = chosen from the selection's size, 1 = the single block, 2 .. 1024
    ListWatch watched[AMM_MAX_WATCH];
    int n_watched = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    Box box;
    bool has_box = true;           // false: amm_create without box edges -- only free-space pair forces and non-periodic terms
    int rank = 0, world = 1;
    std::vector<ForceObj> forces;
    double *d_x = nullptr, *d_v = nullptr;
    const double *d_mass = nullptr;
    double *slots[AMM_MAX_SLOTS] = {nullptr};
    GroupDef groups[AMM_MAX_GROUPS];
    bool profile = false;
    int profile_only = -1;         // >= 0: time only this force id (each timed launch costs two event packets)
    double *d_scratch = nullptr;   // small scratch (reductions)
    double *d_expr_part = nullptr; // block partial sums of amm_expr_eval
    double *d_fscratch = nullptr;  // [n][3] force sink of amm_pair_energy_derivative
    ConstraintSet *constraints = nullptr;   // distance constraints of the System (AMM_OP_CONSTRAIN_*)
    struct VsiteSet *vsites = nullptr;      // virtual sites of the System (vsite.hip); null: none
    std::vector<MinObj *> minimizers;       // amm_min_create (ids are positions, never reused)
    std::vector<ExprDef> exprs;    // registered per-DOF expressions (AMM_OP_EXPR)
    std::vector<BathDef> baths;    // registered baths (AMM_OP_BATH)
    std::vector<StockDef> stocks;  // registered stock integrators (AMM_OP_STOCK)
    std::vector<DrudeStepDef> drude_steps;   // registered Drude steps (AMM_OP_DRUDE_STEP)
    IsoDef iso;                    // isokinetic mode: what AMM_OP_KICK means (amm_iso_define)
    RegDef reg;                    // regulated mode: what AMM_OP_MOVE means (amm_regulated_define)
    unsigned long long expr_seed = 0, expr_counter = 0;
    // ping-pong partners of x, v and the group-0 force buffer for the fused inner RESPA iteration
    double *alt_x = nullptr, *alt_v = nullptr, *alt_f = nullptr;
    bool fuse_inner = true;
    // cut the force-only pair traversal into stretches with / without Lennard-Jones arithmetic (pair.hip).  A row's order of
    // summation then depends on the rows that share its wavefront: results agree to rounding, not bit for bit, between two
    // decompositions.  AMM_SITE_TRIPS=0 (read when the context is created) switches it off -- what the bit-identity tests do.
    bool site_trips = true;
    // amm_set_box: changes so far, those that chose new cell counts for some list, those that freed / allocated device memory or waited
    long long box_changes = 0, box_regrids = 0, box_waits = 0;
    // molecules of amm_mol_define (barostat.hip): CSR on the device, and the molecules of at most AMM_CLUSTER_ATOMS atoms / the longer ones
    int n_mol = 0, n_mol_small = 0, n_mol_long = 0;
    int *d_mol_ptr = nullptr, *d_mol_atoms = nullptr, *d_mol_small = nullptr, *d_mol_long = nullptr;
    long pos_epoch = 0;            // bumped whenever the positions may have changed (see amm_pair_eval_impl)
    double skin_out = -1.0;        // outer Verlet buffer for pair forces created afterwards (<= 0: default)
    void *comm = nullptr;          // ncclComm_t of the library's own communicator (comm.hip), or none
    bool comm_failed = false;      // ... it was aborted after an asynchronous error / a wait that timed out
    double opt_comm_timeout = 0;   // > 0: seconds a wait for the stream may last while a communicator exists before it is aborted (comm.hip:
                                   // amm_comm_wait_impl); 0: no deadline -- the asynchronous error is polled, the work queued may take any time
    double *d_xchg = nullptr;      // caller-owned exchange buffer (amm_bind_exchange): world chunks of 2 x ceil(n/world) x 3 doubles
    long long xchg_doubles = 0;
    PendingExchange pending;
    long long comm_calls = 0, comm_doubles = 0;     // collectives issued / doubles per rank they carried
};

// up to four kicks v <- v + (coef (f -/+ f2)) / m that one launch applies in order (integrate.hip: k_kicks_move; bonded.hip: the
// gather of a term-parallel bond-list evaluation carries the kicks that follow it)
struct KickList {
    const double *f[4], *f2[4];
    int plus[4];
    double coef[4];
    int n;
};

// the neighbour lists whose displacement trigger a kernel that MOVES the atoms evaluates for the positions it writes (their own
// check launch is then skipped: amm_watch_moved).  Passed to kernels by value.
// a list's flag array: [0] "an atom is farther than skin / 2 from where it was at the last build" (rebuild wanted) and, raised by the
// same checks, [AMM_FLAG_FAR] "... farther than the whole skin" (who trusted the list's reference positions with a doubled margin --
// group.hip's candidate walk -- must stop); both cleared by the rebuild
#define AMM_FLAG_FAR 12
struct WatchArgs {
    int n;
    const double *xref[AMM_MAX_WATCH];
    double thr2[AMM_MAX_WATCH];
    int *flags[AMM_MAX_WATCH];
};
// collect them from the context's pair forces (also recorded in ctx->watched) / tell them the positions they watched are current
void amm_collect_watches(amm_ctx *ctx, WatchArgs &W);
void amm_watch_moved(amm_ctx *ctx);

// run_ops.hip: the op scheduler (validated arguments, n_ops > 0, repeat > 0)
int amm_run_ops_impl(amm_ctx *ctx, const amm_op *ops, int n_ops, int repeat, int64_t *cursor);
// families.hip: one force of any type; a new force's id; the object behind an id of family `type` -- any other id is refused with
// the family's wording (who: the entry point, for the families that name it), a live id of another family named by its owner;
// the end of a force whose id stays retired (ids are positions in ctx->forces and are never reused)
int amm_force_eval_dispatch(amm_ctx *ctx, int force_id, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_force_register(amm_ctx *ctx, int type, void *obj);
void *amm_force_lookup(amm_ctx *ctx, int id, int type, const char *who);
int amm_force_release(amm_ctx *ctx, int id, int type, const char *who);
template <class T> T *amm_force_get(amm_ctx *ctx, int id, const char *who = nullptr) {
    return static_cast<T *>(amm_force_lookup(ctx, id, amm_force_type<T>, who));
}
// comm.hip
int amm_comm_unique_id_impl(const char *rccl_path, unsigned char *out);
int amm_comm_init_impl(amm_ctx *ctx, const char *rccl_path, const unsigned char *id_bytes, int rank, int world);
int amm_comm_destroy_impl(amm_ctx *ctx);
int amm_comm_poll_impl(amm_ctx *ctx);                     // asynchronous error of the communicator -> non-zero + message
int amm_comm_wait_impl(amm_ctx *ctx, const char *who);    // bounded hipStreamSynchronize while a communicator exists
int amm_comm_allreduce_impl(amm_ctx *ctx, double *d_buf, size_t count);
int amm_comm_allgather_impl(amm_ctx *ctx, double *d_buf, size_t count_per_rank);
int amm_exchange_finish_impl(amm_ctx *ctx);

// barostat.hip
#define AMM_CLUSTER_ATOMS 8      // molecules of at most this many atoms are scaled one lane each (amm_mol_scale)
int amm_mol_define_impl(amm_ctx *ctx, const int32_t *h_ptr, const int32_t *h_atoms, int n_mol);
int amm_mol_scale_impl(amm_ctx *ctx, double *d_x, double *d_x_saved, const double scale[3]);
int amm_mol_free(amm_ctx *ctx);
// vsite.hip: virtual sites.  place / spread do nothing and return 0 on a context without sites
int amm_vsite_define_impl(amm_ctx *ctx, int n_sites, const int32_t *h_site, const int32_t *h_kind, const int32_t *h_parents,
                          const double *h_weights);
int amm_vsite_place_impl(amm_ctx *ctx, double *d_x);
int amm_vsite_spread_impl(amm_ctx *ctx, const double *d_x, double *d_f);
int amm_vsite_stats_impl(amm_ctx *ctx, int64_t out[4]);
int amm_vsite_free(amm_ctx *ctx);

// group.hip
void amm_small_group_forget(SmallGroup *sg);      // the companion list is about to change under it (amm_set_box): candidates start over
int amm_small_group_setup(amm_ctx *ctx, PairForce *pf, const std::vector<float> &member);
// carry_terms: the launch also evaluates the terms of this (finalized, term-parallel) bond-list set into its parked-force buffer
// own_rows: the caller can take the force's rows from a buffer of the force's own (returned here; nullptr: they are in d_force
// as usual) -- then the launch may walk the candidate atoms only (group.hip: SmallArgs); rows_unused: the caller wants the energy
// alone and d_force is scratch -- candidates again
int amm_small_group_eval_impl(amm_ctx *ctx, PairForce *pf, const double *d_pos, double *d_force, int accumulate, double *d_energy,
                              BondedSet *carry_terms = nullptr, const double **own_rows = nullptr, int rows_unused = 0);
bool amm_small_group_supported(const PairForce *pf);      // k_small_group has an instantiation for the force's family
// energies at K values of lambda of a softcore force on this path (amm_pair_energy_states): d_out[k] += E(d_lambdas[k]), energy only
int amm_small_group_energy_states(amm_ctx *ctx, PairForce *pf, const double *d_pos, const double *d_lambdas, int K, double *d_out);
int amm_small_group_free(SmallGroup *sg);
int amm_small_group_failed(SmallGroup *sg);
int amm_small_group_stats(SmallGroup *sg, int out[2]);
// free.hip: all-pairs evaluation of a free-space pair force (AMM_FREE_SPACE)
int amm_free_eval_impl(amm_ctx *ctx, PairForce *pf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_free_supported(const amm_pair_desc &d, std::string &why);     // 0 + reason: k_pair_free has no instantiation for it
int amm_free_lanes_per_row(int n);
#define AMM_FREE_MAX_ATOMS 32768   // an evaluation is O(n^2): about 10^9 distance tests at the limit
// pair_expr.hip: a force of family AMM_PAIR_EXPR on the per-atom rows of pair.hip
int amm_pair_expr_launch(amm_ctx *ctx, PairForce *pf, const PairArgs &A, dim3 grid, bool en);
void amm_pair_expr_free(PairExpr *px);
// tabulated functions of such a force: does the program read any (sets PairExpr::uses_tables); check them against the program's
// table words and copy them to the force's device allocation (amm_pair_expr_set_tables)
void amm_pair_expr_scan_tables(PairExpr *px);
int amm_pair_expr_tables(amm_ctx *ctx, PairExpr *px, int n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                         const int32_t *offsets, const double *data, int n_data);
// term_expr.hip: a force of type AMM_FORCE_TERM_EXPR
int amm_term_expr_build(amm_ctx *ctx, TermExprForce *tf, const int32_t *h_idx, const double *h_params);   // device arrays + CSR of a new force
int amm_term_expr_upload_params(amm_ctx *ctx, TermExprForce *tf, const double *h_params);
int amm_term_expr_eval_impl(amm_ctx *ctx, TermExprForce *tf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
void amm_term_expr_free(TermExprForce *tf);
// cv.hip: a force of type AMM_FORCE_CV (the inner ids stay the caller's; every inner evaluation goes through amm_force_eval_dispatch)
int amm_cv_create_impl(amm_ctx *ctx, const int32_t *inner_ids, int n_cv, int n_deriv, const int32_t *code, int ncode, const double *consts,
                       int nconst, const double *globals, int nglobal, CvForce **out);
int amm_cv_eval_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_cv_set_globals_impl(amm_ctx *ctx, CvForce *cv, const double *globals, int nglobal);
int amm_cv_set_variables_impl(amm_ctx *ctx, CvForce *cv, const double *values, int n_deriv);
int amm_cv_values_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *h_out);
int amm_cv_energy_derivative_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *d_out);
void amm_cv_free(CvForce *cv);
// compound.hip: a force of type AMM_FORCE_COMPOUND (n_groups > 0: the slots of a bond are weighted centres of groups of atoms)
int amm_compound_create_impl(amm_ctx *ctx, int n_slots, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals,
                             int nglobal, const int32_t *var_kinds, const int32_t *var_slots, int n_vars, const int32_t *h_idx,
                             const double *h_params, int n_bonds, int n_params, int periodic, const int32_t *g_ptr, const int32_t *g_atoms,
                             const double *g_weights, int n_groups, CompoundForce **out);
int amm_compound_eval_impl(amm_ctx *ctx, CompoundForce *cf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_compound_set_globals_impl(amm_ctx *ctx, CompoundForce *cf, const double *globals, int nglobal);
int amm_compound_set_params_impl(amm_ctx *ctx, CompoundForce *cf, const double *h_params, int n_bonds, int n_params);
int amm_compound_set_weights_impl(amm_ctx *ctx, CompoundForce *cf, const double *weights, int n_members);
void amm_compound_free(CompoundForce *cf);
// gb.hip: a force of type AMM_FORCE_GB (rc <= 0: no cutoff)
int amm_gb_create_impl(amm_ctx *ctx, const double *h_q, const double *h_radius, const double *h_scale, double eps_in, double eps_out,
                       double sa_energy, double rc, GbForce **out);
int amm_gb_set_params_impl(amm_ctx *ctx, GbForce *gb, const double *h_q, const double *h_radius, const double *h_scale, double eps_in,
                           double eps_out, double sa_energy, double rc);
int amm_gb_eval_impl(amm_ctx *ctx, GbForce *gb, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_gb_born_radii_impl(amm_ctx *ctx, GbForce *gb, const double *d_pos, double *h_out);
void amm_gb_free(GbForce *gb);
// cmap.hip: a force of type AMM_FORCE_CMAP (h_coeffs: 16 doubles per cell, the maps concatenated; h_idx: n_terms x 8)
int amm_cmap_create_impl(amm_ctx *ctx, int n_maps, const int32_t *h_sizes, const double *h_coeffs, const int32_t *h_map_of_term,
                         const int32_t *h_idx, int n_terms, int periodic, CmapForce **out);
int amm_cmap_set_params_impl(amm_ctx *ctx, CmapForce *cm, const double *h_coeffs, const int32_t *h_map_of_term, int n_maps, int n_terms);
int amm_cmap_eval_impl(amm_ctx *ctx, CmapForce *cm, const double *d_pos, double *d_force, int accumulate, double *d_energy);
void amm_cmap_free(CmapForce *cm);
// custom_gb.hip: a force of type AMM_FORCE_CUSTOM_GB (types / code_ptr / const_ptr: the values' programs, then the energy terms')
int amm_custom_gb_create_impl(amm_ctx *ctx, int n_params, int n_values, int n_terms, const int32_t *types, const int32_t *code,
                              const int32_t *code_ptr, const double *consts, const int32_t *const_ptr, const double *globals, int nglobal,
                              const double *h_params, const int32_t *h_excl, int n_excl, double rc, CustomGbForce **out);
int amm_custom_gb_set_params_impl(amm_ctx *ctx, CustomGbForce *cg, const double *h_params, int n_params, int n_atoms);
int amm_custom_gb_set_globals_impl(amm_ctx *ctx, CustomGbForce *cg, const double *globals, int nglobal);
int amm_custom_gb_set_tables_impl(amm_ctx *ctx, CustomGbForce *cg, int n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                                  const int32_t *offsets, const double *data, int n_data);
int amm_custom_gb_eval_impl(amm_ctx *ctx, CustomGbForce *cg, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_custom_gb_values_impl(amm_ctx *ctx, CustomGbForce *cg, const double *d_pos, double *h_out);
void amm_custom_gb_free(CustomGbForce *cg);
// hbond.hip: a force of type AMM_FORCE_HBOND
int amm_hbond_create_impl(amm_ctx *ctx, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals, int nglobal,
                          const int32_t *var_kinds, const int32_t *var_slots, int n_vars, const int32_t *h_donors, int n_donors,
                          const int32_t *h_acceptors, int n_acceptors, const double *h_dpar, int n_dpar, const double *h_apar, int n_apar,
                          const int32_t *h_excl, int n_excl, double rc, int periodic, HbondForce **out);
int amm_hbond_set_params_impl(amm_ctx *ctx, HbondForce *hb, const double *h_dpar, int n_donors, int n_dpar, const double *h_apar, int n_acceptors,
                              int n_apar);
int amm_hbond_set_globals_impl(amm_ctx *ctx, HbondForce *hb, const double *globals, int nglobal);
int amm_hbond_eval_impl(amm_ctx *ctx, HbondForce *hb, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_hbond_stats_impl(amm_ctx *ctx, HbondForce *hb, int64_t out[4]);
void amm_hbond_free(HbondForce *hb);
// manyparticle.hip: a force of type AMM_FORCE_MANY_PARTICLE
int amm_many_create_impl(amm_ctx *ctx, const int32_t *code, int ncode, const double *consts, int nconst, const double *globals, int nglobal,
                         const int32_t *var_kinds, const int32_t *var_slots, int n_vars, int n_particles, const double *h_params, int n_params,
                         const int32_t *h_types, int n_types, const int32_t *h_perm, const int32_t *h_excl, int n_excl, double rc, int periodic,
                         int central, ManyForce **out);
int amm_many_set_params_impl(amm_ctx *ctx, ManyForce *mf, const double *h_params, int n_particles, int n_params, const int32_t *h_types, int n_types,
                             const int32_t *h_perm);
int amm_many_set_globals_impl(amm_ctx *ctx, ManyForce *mf, const double *globals, int nglobal);
int amm_many_eval_impl(amm_ctx *ctx, ManyForce *mf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_many_stats_impl(amm_ctx *ctx, ManyForce *mf, int64_t out[5]);
int amm_many_overflow(ManyForce *mf, int *need, int *capacity);   // amm_check: 1 when a neighbour row overflowed, 0 when none did, -1 on a HIP error
void amm_many_free(ManyForce *mf);
// rmsd.hip: a force of type AMM_FORCE_RMSD (h_ref: the reference rows of the listed particles, in the list's order)
int amm_rmsd_create_impl(amm_ctx *ctx, const int32_t *h_particles, int n_sel, const double *h_ref, RmsdForce **out);
int amm_rmsd_set_reference_impl(amm_ctx *ctx, RmsdForce *rf, const int32_t *h_particles, int n_sel, const double *h_ref);
int amm_rmsd_eval_impl(amm_ctx *ctx, RmsdForce *rf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_rmsd_stats_impl(RmsdForce *rf, int64_t out[4]);
void amm_rmsd_free(RmsdForce *rf);
// gayberne.hip: a force of type AMM_FORCE_GAYBERNE (the tables are those of amm_gayberne_create, include/atomsmm_hip.h)
int amm_gayberne_create_impl(amm_ctx *ctx, const int32_t *h_active, int n_act, const int32_t *h_axes, const double *h_par, const int32_t *h_ex_ptr,
                             const int32_t *h_ex_col, const double *h_ex_par, const int32_t *h_rev_ptr, const int32_t *h_rev_src, double rc,
                             double rs, int periodic, GayBerneForce **out);
int amm_gayberne_set_params_impl(amm_ctx *ctx, GayBerneForce *gf, const double *h_par, int n_act, const double *h_ex_par, int n_ex);
int amm_gayberne_eval_impl(amm_ctx *ctx, GayBerneForce *gf, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_gayberne_stats_impl(amm_ctx *ctx, GayBerneForce *gf, int64_t out[5]);
void amm_gayberne_free(GayBerneForce *gf);
// drude.hip: a force of type AMM_FORCE_DRUDE (the tables are those of amm_drude_create, include/atomsmm_hip.h) and the step of
// AMM_OP_DRUDE_STEP
int amm_drude_create_impl(amm_ctx *ctx, const int32_t *h_idx, const double *h_par, int n_spring, const int32_t *h_pent, const double *h_thole,
                          int n_pair, int periodic, DrudeForce **out);
int amm_drude_set_params_impl(amm_ctx *ctx, DrudeForce *df, const int32_t *h_idx, const double *h_par, int n_spring, const int32_t *h_pent,
                              const double *h_thole, int n_pair);
int amm_drude_eval_impl(amm_ctx *ctx, DrudeForce *df, const double *d_pos, double *d_force, int accumulate, double *d_energy);
void amm_drude_free(DrudeForce *df);
int amm_drude_step_define_impl(amm_ctx *ctx, const int32_t *h_pairs, int n_pairs, double dt, double friction, double kT, double drude_friction,
                               double drude_kT, double max_distance, int *id);
int amm_drude_step_impl(amm_ctx *ctx, const DrudeStepDef &D, const double *d_f, unsigned long long counter);
int amm_drude_step_flagged(amm_ctx *ctx);
void amm_drude_steps_free(amm_ctx *ctx);
// implemented in pair.hip / cells.hip / bonded.hip / integrate.hip
int amm_pair_build_consts(const amm_pair_desc &d, PairConsts &pc);
int amm_pair_eval_impl(amm_ctx *ctx, PairForce *pf, const double *d_pos, double *d_force, int accumulate,
                       double *d_energy, PairForce *guest = nullptr, double *g_force = nullptr, int g_accumulate = 0,
                       int exchange = 0);
bool amm_pair_can_eval_dual(amm_ctx *ctx, PairForce *guest, PairForce *host);
bool amm_pair_can_fuse_discount(amm_ctx *ctx, PairForce *guest, PairForce *host);
int amm_pair_free(PairForce *pf);            // (like every family's free: the device memory and the object)
// amm_set_box: drop the per-atom rows and their capacities and choose the cell counts again for the context's box (the next evaluation
// builds and sizes them as the first one did); frees device memory -- the caller has waited for the stream
int amm_pair_regrid(amm_ctx *ctx, PairForce *pf);
int amm_pair_build_table(PairForce *pf);
int amm_pair_count_within_impl(amm_ctx *ctx, PairForce *pf, const double *d_pos, double r_within, long long *count);
const char *amm_kernel_revision_impl();
int amm_pair_table_check_impl(const amm_pair_desc &d, double site_sigma, double site_eps, double site_q, long long out[8]);
int amm_bonded_eval_impl(amm_ctx *ctx, BondedSet *bs, const double *d_pos, double *d_force, int accumulate,
                         double *d_energy);
int amm_bonded_finalize_impl(amm_ctx *ctx, BondedSet *bs);
// EVAL of a term-parallel set followed by kicks (and a move): the gather launch applies them (bit-identical to the separate ops)
int amm_bonded_eval_kicks_impl(amm_ctx *ctx, BondedSet *bs, const double *d_pos, double *d_force, int accumulate, const KickList &K,
                               int with_move, double dcoef, int terms_done = 0, const double *pair_rows = nullptr);
int amm_bonded_free(BondedSet *bs);
// (with_move: the launch also evaluates the displacement triggers of the context's lists; the caller bumps pos_epoch and calls
// amm_watch_moved)
int amm_kicks_move_impl(amm_ctx *ctx, const double *const *fa, const double *const *fb, const int *plus, const double *coef, int nk,
                        int with_move, double dcoef);
int amm_inner_components_impl(amm_ctx *ctx, BondedSet *bs, double *x, double *v, double *f0, int npre, const double *const *pre_a,
                              const double *const *pre_b, const double *pre_coef, const int *pre_plus, double c1, double d,
                              double c2, int niter, const BathDef *bath = nullptr, double d2 = 0.0);
int amm_bath_impl(amm_ctx *ctx, const BathDef &bath, double *d_v, unsigned long long counter);
int amm_stock_step_impl(amm_ctx *ctx, const StockDef &sd, const double *d_f, unsigned long long counter);       // stock.hip
int amm_isokick_impl(amm_ctx *ctx, double *d_v, const double *d_f, const double *d_f2, int plus, const double *d_mass, double coef);
int amm_constraints_create_impl(amm_ctx *ctx, const int32_t *h_pairs, const double *h_dist, int n_cons, double tol,
                                ConstraintSet **out);
int amm_constraints_save_reference(amm_ctx *ctx, ConstraintSet *cs, const double *d_x);
int amm_constrain_positions(amm_ctx *ctx, ConstraintSet *cs, double *d_x);
int amm_constrain_velocities(amm_ctx *ctx, ConstraintSet *cs, const double *d_x, double *d_v);
int amm_constraints_set_tolerance_impl(ConstraintSet *cs, double tol);
int amm_constraints_failed(amm_ctx *ctx, ConstraintSet *cs);
int amm_constraints_free(ConstraintSet *cs);
int amm_fused_inner_impl(amm_ctx *ctx, BondedSet *bs, const double *x_in, const double *v_in, const double *f_in,
                         double *x_out, double *v_out, double *f_out, double c1, double d, double c2);
int amm_pme_create_impl(amm_ctx *ctx, double alpha, const int *K, double Kc, const double *h_q, PmeForce **out);
int amm_pme_set_charges_impl(amm_ctx *ctx, PmeForce *pm, const double *h_q);
int amm_pme_eval_impl(amm_ctx *ctx, PmeForce *pm, const double *d_pos, double *d_force, int accumulate, double *d_energy);
int amm_pme_set_sliced_impl(PmeForce *pm, int on);
int amm_pme_free(PmeForce *pm);
int amm_expr_eval_scalar_impl(amm_ctx *ctx, const int32_t *code, int n_code, const double *consts, int n_consts, double *d_scalars,
                              int n_scalars);
int amm_expr_eval_impl(amm_ctx *ctx, const int32_t *code, int n_code, const double *consts, int n_consts, const double *globals,
                       int n_globals, unsigned long long seed, unsigned long long counter, double *d_dst, double *d_sum);
int amm_kick_impl(amm_ctx *ctx, double *d_v, const double *d_f, const double *d_f2, int plus, const double *d_mass, double coef);
int amm_combine_impl(amm_ctx *ctx, double *d_dst, const double *d_a, const double *d_b, double coef);
int amm_move_impl(amm_ctx *ctx, double *d_x, const double *d_v, double coef);
int amm_copy_impl(amm_ctx *ctx, double *d_dst, const double *d_src);
int amm_mvv_impl(amm_ctx *ctx, const double *d_v, const double *d_m, double *d_out);
int amm_reduce_add(amm_ctx *ctx, const double *d_part, int n, double scale, double *d_out);
int amm_min_create_impl(amm_ctx *ctx, int memory, double max_step, int force_input, const double *d_mass, double *d_scalars, int *id);
int amm_min_release_impl(amm_ctx *ctx, int id);
int amm_min_free(MinObj *mo);
int amm_min_begin_impl(amm_ctx *ctx, int id, const double *d_x, const double *d_g);
int amm_min_advance_impl(amm_ctx *ctx, int id, const double *d_x, const double *d_g);
int amm_min_trial_impl(amm_ctx *ctx, int id, double alpha, double *d_x_out);
int amm_min_scalars_impl(amm_ctx *ctx, int id, double out[8]);
int amm_min_stats_impl(amm_ctx *ctx, int id, int64_t out[8]);
int amm_min_read_impl(amm_ctx *ctx, int id, int what, double *h_out);
