"""ctypes binding of include/atomsmm_hip.h (libatomsmm_hip.so, gfx950).

There is NO CPU fallback: if the shared library is missing or no HIP device is visible, every entry
point raises.  Device memory, streams and collectives come from torch (plumbing only).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AMM_LIB') or os.path.join(HERE, 'libatomsmm_hip.so')      # AMM_LIB: an experimental build (kernel tuning)

NEAR_NONE, NEAR_SHIFT, NEAR_FSWITCH, DAMPED, NONBONDED, SOFTCORE, LJ_VIRIAL = range(7)
PAIR_EXPR = 7      # any other CustomNonbondedForce text: compiled (expr.compile_pair) and interpreted per pair (csrc/pair_expr.hip)
GUARD_RC0, COULOMB_EWALD, COULOMB_RF, SWITCH, NO_SHIFT, GROUP_LJ, GROUP_Q = 1, 2, 4, 8, 16, 32, 64
FREE_SPACE = 128   # NoCutoff / CutoffNonPeriodic: all pairs, no box, no list (csrc/free.hip)
TERM_BOND, TERM_ANGLE, TERM_TORSION, TERM_EXTERNAL = range(4)     # amm_term_kind: the variable of a term-expression force
CVAR_X, CVAR_Y, CVAR_Z, CVAR_DISTANCE, CVAR_ANGLE, CVAR_DIHEDRAL = range(6)     # amm_compound_var: a variable of a compound-bond force
BOND_HARMONIC, ANGLE_HARMONIC, BOND_LJC, BOND_NEAR, TORSION_PERIODIC, BOND_EWALD_EXCL = range(6)
BOND_VIRIAL_HARMONIC, BOND_VIRIAL_LJ = 6, 7
OP_EVAL, OP_KICK, OP_MOVE, OP_COPY, OP_COMBINE, OP_EXPR, OP_BATH = 1, 2, 3, 4, 5, 6, 7
OP_SAVE_REF, OP_CONSTRAIN_X, OP_CONSTRAIN_V = 8, 9, 10
OP_ALLREDUCE = 11
OP_STOCK = 12
OP_DRUDE_STEP = 13
STOCK_VERLET, STOCK_LANGEVIN_MIDDLE, STOCK_LANGEVIN, STOCK_BROWNIAN = range(4)   # amm_stock_define kinds
VSITE_AVERAGE2, VSITE_AVERAGE3, VSITE_OUT_OF_PLANE = range(3)                     # amm_vsite_define kinds
EXCHANGE_REDUCE, EXCHANGE_GATHER = 0, 1
COMM_ID_BYTES = 128
MAX_SLOTS, SLOT_X, SLOT_V = 64, 62, 63
MAX_STATES = 64  # amm_pair_energy_states
GROUP_ALL = 32   # pseudo-group of the force symbol `f` (all groups)
KC = 138.935456   # forces.py:407
ARITY = {BOND_HARMONIC: 2, ANGLE_HARMONIC: 3, BOND_LJC: 2, BOND_NEAR: 2, TORSION_PERIODIC: 4, BOND_EWALD_EXCL: 2,
         BOND_VIRIAL_HARMONIC: 2, BOND_VIRIAL_LJ: 2}
NPAR = {BOND_HARMONIC: 2, ANGLE_HARMONIC: 2, BOND_LJC: 3, BOND_NEAR: 3, TORSION_PERIODIC: 3, BOND_EWALD_EXCL: 1,
        BOND_VIRIAL_HARMONIC: 2, BOND_VIRIAL_LJ: 3}

RULE_NAMES = ('plain', 'defer_trailing_kicks', 'inner_components', 'fused_inner', 'dual_eval', 'terms_kicks', 'kicks_move',
              'plan_offers')      # amm_run_rule_stats: out[0..7]

EXPORTS = [
    'amm_abi_version', 'amm_last_error', 'amm_create', 'amm_destroy', 'amm_set_stream', 'amm_set_slice',
    'amm_synchronize', 'amm_check', 'amm_pair_create', 'amm_pair_set_params', 'amm_pair_share_list', 'amm_bonded_create',
    'amm_bonded_add_terms', 'amm_bonded_finalize', 'amm_bonded_set_sliced', 'amm_bonded_release', 'amm_bonded_stats', 'amm_force_eval', 'amm_kick',
    'amm_move', 'amm_copy', 'amm_mvv', 'amm_bind_state', 'amm_bind_buffer', 'amm_group_define', 'amm_run_ops',
    'amm_set_fuse_inner', 'amm_set_outer_skin',
    'amm_pair_get_stats', 'amm_profile_enable', 'amm_profile_read', 'amm_pair_count_within', 'amm_pair_row_padding', 'amm_pair_guest_factor', 'amm_kernel_revision', 'amm_pair_table_check',
    'amm_pme_create', 'amm_pme_set_charges', 'amm_pme_set_sliced', 'amm_pair_set_lambda', 'amm_pair_set_lambda_dev', 'amm_expr_eval', 'amm_expr_eval_scalar', 'amm_expr_define', 'amm_expr_seed', 'amm_bath_define', 'amm_stock_define', 'amm_bath_define_nhl', 'amm_bath_define_sin', 'amm_iso_define', 'amm_regulated_define', 'amm_bath_define_regulated', 'amm_pair_energy_derivative', 'amm_constraints_create', 'amm_constraints_set_tolerance', 'amm_pair_set_scale',
    'amm_comm_unique_id', 'amm_comm_init', 'amm_comm_destroy', 'amm_comm_allreduce', 'amm_comm_stats', 'amm_group_set_exchange', 'amm_bind_exchange', 'amm_exchange_finish',
    'amm_set_option', 'amm_positions_changed', 'amm_exchange_per', 'amm_run_stats', 'amm_run_ops_from', 'amm_exchange_pending',
    'amm_pair_energy_states',
    'amm_min_create', 'amm_min_release', 'amm_min_begin', 'amm_min_advance', 'amm_min_trial', 'amm_min_scalars', 'amm_min_stats',
    'amm_min_read',
    'amm_set_box', 'amm_box_stats', 'amm_mol_define', 'amm_mol_scale',
    'amm_pair_expr_create', 'amm_pair_expr_set_globals', 'amm_pair_expr_set_tables',
    'amm_term_expr_create', 'amm_term_expr_set_globals', 'amm_term_expr_set_params', 'amm_term_expr_release',
    'amm_cv_create', 'amm_cv_set_globals', 'amm_cv_set_variables', 'amm_cv_values', 'amm_cv_energy_derivative', 'amm_cv_release',
    'amm_compound_create', 'amm_compound_set_globals', 'amm_compound_set_params', 'amm_compound_set_weights', 'amm_compound_release',
    'amm_run_rule_stats',
    'amm_gb_create', 'amm_gb_set_params', 'amm_gb_born_radii', 'amm_gb_release',
    'amm_cmap_create', 'amm_cmap_set_params', 'amm_cmap_release',
    'amm_custom_gb_create', 'amm_custom_gb_set_params', 'amm_custom_gb_set_globals', 'amm_custom_gb_set_tables', 'amm_custom_gb_values',
    'amm_custom_gb_release',
    'amm_hbond_create', 'amm_hbond_set_params', 'amm_hbond_set_globals', 'amm_hbond_stats', 'amm_hbond_release',
    'amm_many_create', 'amm_many_set_params', 'amm_many_set_globals', 'amm_many_stats', 'amm_many_release',
    'amm_rmsd_create', 'amm_rmsd_set_reference', 'amm_rmsd_stats', 'amm_rmsd_release',
    'amm_gayberne_create', 'amm_gayberne_set_params', 'amm_gayberne_stats', 'amm_gayberne_release',
    'amm_drude_create', 'amm_drude_set_params', 'amm_drude_release', 'amm_drude_step_define',
    'amm_vsite_define', 'amm_vsite_place', 'amm_vsite_spread', 'amm_vsite_stats',
]


class PairDesc(C.Structure):
    _fields_ = [('family', C.c_int32), ('flags', C.c_int32), ('degree', C.c_int32), ('pad_', C.c_int32),
                ('sign', C.c_double), ('rc', C.c_double), ('rswitch', C.c_double), ('rc0', C.c_double),
                ('rs0', C.c_double), ('alpha', C.c_double), ('Kc', C.c_double), ('krf', C.c_double),
                ('crf', C.c_double)]


class Op(C.Structure):
    _fields_ = [('op', C.c_int32), ('a', C.c_int32), ('b', C.c_int32), ('c', C.c_int32), ('coef', C.c_double)]


class PairStats(C.Structure):
    _fields_ = [('n_builds', C.c_int64), ('n_evals', C.c_int64), ('n_list_pairs', C.c_int64),
                ('n_slice_atoms', C.c_int64), ('capacity', C.c_int32), ('max_neighbors', C.c_int32),
                ('lanes_per_atom', C.c_int32), ('n_cells', C.c_int32), ('rlist', C.c_double),
                ('shares_list', C.c_int32), ('list_kind', C.c_int32), ('n_outer_builds', C.c_int64),
                ('n_outer_pairs', C.c_int64), ('rlist_outer', C.c_double), ('tab_error', C.c_double),
                ('has_table', C.c_int32), ('rode_along', C.c_int32),
                ('has_site_table', C.c_int32), ('n_rest_atoms', C.c_int32), ('site_tab_error', C.c_double),
                ('n_candidates', C.c_int32), ('n_candidate_walks', C.c_int32), ('chargeless', C.c_int32), ('build_split', C.c_int32)]


def slice_per(n, world):
    """Slots of the cell-sorted order per rank: whole molecules of three (csrc/amm_ctx.h: amm_slice_per)."""
    return 3 * (((n + 2) // 3 + world - 1) // world)


def pair_desc(family, rc, rc0=0.0, rs0=0.0, rswitch=0.0, alpha=0.0, degree=1, flags=0, sign=1.0, Kc=KC,
              krf=0.0, crf=0.0):
    return PairDesc(int(family), int(flags), int(degree), 0, float(sign), float(rc), float(rswitch), float(rc0),
                    float(rs0), float(alpha), float(Kc), float(krf), float(crf))


class HipError(RuntimeError):
    pass


class _LiveSet:
    """Identity set of the open contexts (weak references: a context that is garbage-collected closes itself)."""

    def __init__(self):
        import weakref
        self._refs = weakref.WeakValueDictionary()

    def add(self, obj):
        self._refs[id(obj)] = obj

    def discard(self, obj):
        self._refs.pop(id(obj), None)

    def close_all(self):
        for obj in list(self._refs.values()):
            try:
                obj.close()
            except Exception:
                pass


_LIVE = _LiveSet()
import atexit  # noqa: E402
atexit.register(_LIVE.close_all)


_LIB = None


def kernel_revision():
    return lib().amm_kernel_revision().decode()


def pair_table_check(desc, site_sigma=0.0, site_eps=0.0, site_q=0.0):
    """Host-only (no GPU): the radial tables of `desc` (pair_desc) built as amm_pair_create builds them, and the unclamped interval
    index at the ends and boundaries of the range a counting pair can have.  -> dict(nint, ss_first, points, bad, idx_min, idx_max,
    n_below_kink, fine); `bad` must be 0."""
    out = (C.c_int64 * 8)()
    _chk(lib().amm_pair_table_check(C.byref(desc), float(site_sigma), float(site_eps), float(site_q), out))
    return dict(zip(('nint', 'ss_first', 'points', 'bad', 'idx_min', 'idx_max', 'n_below_kink', 'fine'), (int(v) for v in out)))


def lib():
    """Load libatomsmm_hip.so; raises HipError when it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HipError('libatomsmm_hip.so not found at %s: build it with `python -m atomsmm_amd.build` '
                           '(hipcc --offload-arch=gfx950). The HIP path has no CPU fallback.' % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.amm_kernel_revision.restype = C.c_char_p
        revision = L.amm_kernel_revision().decode()
        if revision.endswith('-tune') and os.environ.get('AMM_ALLOW_TUNE') != '1':
            # a kernel-tuning / measurement build (scripts/build_variant.sh): only part of the kernels, or kernels with arithmetic
            # removed -- never what a bench line or a test may run on
            raise HipError('%s is a tuning build (kernel revision %s): rebuild with `python -m atomsmm_amd.build --force`, or set '
                           'AMM_ALLOW_TUNE=1 for a probe script' % (LIB_PATH, revision))
        L.amm_abi_version.restype = C.c_int
        L.amm_last_error.restype = C.c_char_p
        L.amm_create.argtypes = [C.c_int32, dp, C.c_int32, vp, C.POINTER(vp)]
        L.amm_destroy.argtypes = [vp]
        L.amm_set_stream.argtypes = [vp, vp]
        L.amm_set_slice.argtypes = [vp, C.c_int32, C.c_int32]
        L.amm_synchronize.argtypes = [vp]
        L.amm_comm_unique_id.argtypes = [C.c_char_p, C.c_char_p]
        L.amm_comm_init.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]
        L.amm_comm_allreduce.argtypes = [vp, vp, C.c_int64]
        L.amm_comm_destroy.argtypes = [vp]
        L.amm_comm_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        L.amm_run_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        L.amm_run_rule_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        L.amm_group_set_exchange.argtypes = [vp, C.c_int32, C.c_int32]
        L.amm_bind_exchange.argtypes = [vp, vp, C.c_int64]
        L.amm_exchange_finish.argtypes = [vp]
        L.amm_exchange_pending.argtypes = [vp, C.POINTER(C.c_int32)]
        L.amm_check.argtypes = [vp]
        L.amm_pair_create.argtypes = [vp, C.POINTER(PairDesc), dp, dp, dp, ip, C.c_int32, C.c_double, ip]
        L.amm_pair_set_params.argtypes = [vp, C.c_int32, dp, dp, dp]
        L.amm_pair_expr_create.argtypes = [vp, C.POINTER(PairDesc), ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, dp, dp, dp, ip, C.c_int32, C.c_double, ip]
        L.amm_pair_expr_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_pair_expr_set_tables.argtypes = [vp, C.c_int32, C.c_int32, ip, ip, dp, ip, dp, C.c_int32]
        L.amm_term_expr_create.argtypes = [vp, C.c_int32, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip, dp, C.c_int32, C.c_int32, C.c_int32, ip]
        L.amm_term_expr_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_term_expr_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32]
        L.amm_term_expr_release.argtypes = [vp, C.c_int32]
        L.amm_compound_create.argtypes = [vp, C.c_int32, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip, ip, C.c_int32, ip, dp, C.c_int32, C.c_int32,
                                          C.c_int32, ip, ip, dp, C.c_int32, ip]
        L.amm_compound_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_compound_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32]
        L.amm_compound_set_weights.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_compound_release.argtypes = [vp, C.c_int32]
        L.amm_gb_create.argtypes = [vp, dp, dp, dp, C.c_double, C.c_double, C.c_double, C.c_double, ip]
        L.amm_gb_set_params.argtypes = [vp, C.c_int32, dp, dp, dp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.amm_gb_born_radii.argtypes = [vp, C.c_int32, vp, dp]
        L.amm_gb_release.argtypes = [vp, C.c_int32]
        L.amm_cmap_create.argtypes = [vp, C.c_int32, ip, dp, ip, ip, C.c_int32, C.c_int32, ip]
        L.amm_cmap_set_params.argtypes = [vp, C.c_int32, dp, ip, C.c_int32, C.c_int32]
        L.amm_cmap_release.argtypes = [vp, C.c_int32]
        L.amm_custom_gb_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, ip, ip, ip, dp, ip, dp, C.c_int32, dp, ip, C.c_int32, C.c_double, ip]
        L.amm_custom_gb_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32]
        L.amm_custom_gb_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_custom_gb_set_tables.argtypes = [vp, C.c_int32, C.c_int32, ip, ip, dp, ip, dp, C.c_int32]
        L.amm_custom_gb_values.argtypes = [vp, C.c_int32, vp, dp]
        L.amm_custom_gb_release.argtypes = [vp, C.c_int32]
        L.amm_hbond_create.argtypes = [vp, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip, ip, C.c_int32, ip, C.c_int32, ip, C.c_int32, dp, C.c_int32,
                                       dp, C.c_int32, ip, C.c_int32, C.c_double, C.c_int32, ip]
        L.amm_hbond_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32, dp, C.c_int32, C.c_int32]
        L.amm_hbond_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_hbond_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_hbond_release.argtypes = [vp, C.c_int32]
        L.amm_many_create.argtypes = [vp, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip, ip, C.c_int32, C.c_int32, dp, C.c_int32, ip, C.c_int32, ip,
                                      ip, C.c_int32, C.c_double, C.c_int32, C.c_int32, ip]
        L.amm_many_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32, ip, C.c_int32, ip]
        L.amm_many_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_many_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_many_release.argtypes = [vp, C.c_int32]
        L.amm_rmsd_create.argtypes = [vp, ip, C.c_int32, dp, ip]
        L.amm_rmsd_set_reference.argtypes = [vp, C.c_int32, ip, C.c_int32, dp]
        L.amm_rmsd_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_rmsd_release.argtypes = [vp, C.c_int32]
        L.amm_gayberne_create.argtypes = [vp, ip, C.c_int32, ip, dp, ip, ip, dp, ip, ip, C.c_double, C.c_double, C.c_int32, ip]
        L.amm_gayberne_set_params.argtypes = [vp, C.c_int32, dp, C.c_int32, dp, C.c_int32]
        L.amm_gayberne_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_gayberne_release.argtypes = [vp, C.c_int32]
        L.amm_drude_create.argtypes = [vp, ip, dp, C.c_int32, ip, dp, C.c_int32, C.c_int32, ip]
        L.amm_drude_set_params.argtypes = [vp, C.c_int32, ip, dp, C.c_int32, ip, dp, C.c_int32]
        L.amm_drude_release.argtypes = [vp, C.c_int32]
        L.amm_drude_step_define.argtypes = [vp, ip, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, ip]
        L.amm_cv_create.argtypes = [vp, ip, C.c_int32, C.c_int32, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip]
        L.amm_cv_set_globals.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_cv_set_variables.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.amm_cv_values.argtypes = [vp, C.c_int32, vp, dp]
        L.amm_cv_energy_derivative.argtypes = [vp, C.c_int32, vp, vp]
        L.amm_cv_release.argtypes = [vp, C.c_int32]
        L.amm_pair_share_list.argtypes = [vp, C.c_int32, C.c_int32]
        L.amm_bonded_create.argtypes = [vp, ip]
        L.amm_bonded_add_terms.argtypes = [vp, C.c_int32, C.c_int32, ip, dp, C.c_int32, C.c_int32, C.POINTER(PairDesc)]
        L.amm_bonded_finalize.argtypes = [vp, C.c_int32]
        L.amm_bonded_set_sliced.argtypes = [vp, C.c_int32, C.c_int32]
        L.amm_bonded_release.argtypes = [vp, C.c_int32]
        L.amm_bonded_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_force_eval.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp]
        L.amm_kick.argtypes = [vp, vp, vp, vp, C.c_int32, vp, C.c_double]
        L.amm_move.argtypes = [vp, vp, vp, C.c_double]
        L.amm_copy.argtypes = [vp, vp, vp]
        L.amm_mvv.argtypes = [vp, vp, vp, vp]
        L.amm_bind_state.argtypes = [vp, vp, vp, vp]
        L.amm_bind_buffer.argtypes = [vp, C.c_int32, vp]
        L.amm_group_define.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_int32]
        L.amm_run_ops.argtypes = [vp, C.POINTER(Op), C.c_int32, C.c_int32]
        L.amm_run_ops_from.argtypes = [vp, C.POINTER(Op), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_set_fuse_inner.argtypes = [vp, C.c_int32]
        L.amm_set_outer_skin.argtypes = [vp, C.c_double]
        L.amm_pair_get_stats.argtypes = [vp, C.c_int32, C.POINTER(PairStats)]
        L.amm_profile_enable.argtypes = [vp, C.c_int32]
        L.amm_pair_count_within.argtypes = [vp, C.c_int32, vp, C.c_double, C.POINTER(C.c_int64)]
        L.amm_pair_row_padding.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_pair_guest_factor.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
        L.amm_kernel_revision.restype = C.c_char_p
        L.amm_kernel_revision.argtypes = []
        L.amm_pair_table_check.argtypes = [C.POINTER(PairDesc), C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)]
        L.amm_profile_read.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp]
        L.amm_pme_create.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, dp, ip]
        L.amm_pme_set_charges.argtypes = [vp, C.c_int32, dp]
        L.amm_pme_set_sliced.argtypes = [vp, C.c_int32, C.c_int32]
        L.amm_pair_set_lambda.argtypes = [vp, C.c_int32, C.c_double]
        L.amm_pair_set_lambda_dev.argtypes = [vp, C.c_int32, vp]
        L.amm_expr_eval_scalar.argtypes = [vp, ip, C.c_int32, dp, C.c_int32, vp, C.c_int32]
        L.amm_pair_set_scale.argtypes = [vp, C.c_int32, C.c_double]
        L.amm_expr_define.argtypes = [vp, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip]
        L.amm_expr_seed.argtypes = [vp, C.c_uint64]
        L.amm_constraints_create.argtypes = [vp, ip, dp, C.c_int32, C.c_double]
        L.amm_constraints_set_tolerance.argtypes = [vp, C.c_double]
        L.amm_pair_energy_derivative.argtypes = [vp, C.c_int32, vp, vp]
        L.amm_pair_energy_states.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp]
        L.amm_bath_define.argtypes = [vp, C.c_double, C.c_double, ip]
        L.amm_stock_define.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_double, ip]
        L.amm_bath_define_nhl.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, ip]
        L.amm_bath_define_sin.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, ip]
        L.amm_iso_define.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_int32]
        L.amm_regulated_define.argtypes = [vp, C.c_int32, C.c_double, C.c_double]
        L.amm_bath_define_regulated.argtypes = [vp, C.c_int32, C.c_int32] + [C.c_double] * 8 + [C.c_int32, ip]
        L.amm_set_option.argtypes = [vp, C.c_char_p, C.c_double]
        L.amm_positions_changed.argtypes = [vp]
        L.amm_exchange_per.argtypes = [vp, ip]
        L.amm_expr_eval.argtypes = [vp, ip, C.c_int32, dp, C.c_int32, dp, C.c_int32, C.c_uint64, C.c_uint64, vp, vp]
        L.amm_min_create.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, vp, vp, ip]
        L.amm_min_release.argtypes = [vp, C.c_int32]
        L.amm_min_begin.argtypes = [vp, C.c_int32, vp, vp]
        L.amm_min_advance.argtypes = [vp, C.c_int32, vp, vp]
        L.amm_min_trial.argtypes = [vp, C.c_int32, C.c_double, vp]
        L.amm_min_scalars.argtypes = [vp, C.c_int32, dp]
        L.amm_min_stats.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        L.amm_min_read.argtypes = [vp, C.c_int32, C.c_int32, dp]
        L.amm_set_box.argtypes = [vp, dp]
        L.amm_box_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        L.amm_mol_define.argtypes = [vp, ip, ip, C.c_int32]
        L.amm_mol_scale.argtypes = [vp, vp, vp, dp]
        L.amm_vsite_define.argtypes = [vp, C.c_int32, ip, ip, ip, dp]
        L.amm_vsite_place.argtypes = [vp, vp]
        L.amm_vsite_spread.argtypes = [vp, vp, vp]
        L.amm_vsite_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        for name in EXPORTS:
            if name not in ('amm_last_error', 'amm_kernel_revision'):
                getattr(L, name).restype = C.c_int
        L.amm_last_error.restype = C.c_char_p
        L.amm_kernel_revision.restype = C.c_char_p
        _LIB = _Serialised(L)
    return _LIB


class _Serialised:
    """The loaded library with ONE caller at a time: ctypes releases the GIL during a call, and the library's host code (launch
    caches, upload flags) is not written for two threads inside it at once.  Matters only for engine.LocalWorld -- ranks as threads of
    one process -- and costs a quarter of a microsecond per call otherwise."""

    def __init__(self, library):
        import threading
        self._library = library
        self._lock = threading.RLock()

    def __getattr__(self, name):
        fn = getattr(self._library, name)          # (AttributeError for a missing symbol, as ctypes raises it)
        lock = self._lock

        def call(*args):
            with lock:
                return fn(*args)
        self.__dict__[name] = call
        return call


def _chk(rc):
    if rc != 0:
        raise HipError(lib().amm_last_error().decode())


def _hd(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _hi(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _globals(globals_):
    """(pointer, count) of the values of a program's globals (a pointer keeps its array alive)."""
    g_, gp = _hd(globals_ if len(globals_) else [0.0])
    return gp, len(globals_)


def _program(code, consts, globals_):
    """The six arguments every text-driven entry point takes for its program: code, constants, globals, each with its count."""
    c_, cp = _hi(np.asarray(code, dtype=np.int32).reshape(-1))
    k_, kp = _hd(consts if len(consts) else [0.0])
    return (cp, len(c_), kp, len(consts)) + _globals(globals_)


def _var_table(var_kinds, var_slots):
    """(kinds, slots n_vars x 4 padded with 0, n_vars) of a variable table (expr.compile_compound / compile_hbond / compile_many_particle)."""
    n_vars = len(var_kinds)
    slots = np.zeros((max(n_vars, 1), 4), dtype=np.int32)
    for k, row in enumerate(var_slots):
        slots[k, :len(row)] = row
    return _hi(var_kinds if n_vars else [0])[1], _hi(slots)[1], n_vars


def _param_major(params, n, keep_rows=False):
    """(pointer, n_params) of a parameter-major array n_params x n.  Anything empty: no parameters -- or, with keep_rows, those
    of a 2-D array without columns (a force without terms whose text still reads its parameters)."""
    par = np.asarray(params, dtype=np.float64)
    if n and par.size:
        par = par.reshape(-1, n)
    else:
        par = np.zeros((par.shape[0] if keep_rows and not n and par.ndim == 2 else 0, n))
    return _hd(par if par.size else [0.0])[1], len(par)


def _pairs(excl_pairs):
    """(pointer, count) of a list of index pairs (None: none)."""
    ex = np.zeros((0, 2), np.int32) if excl_pairs is None else np.asarray(excl_pairs, dtype=np.int32).reshape(-1, 2)
    return _hi(ex if len(ex) else [0])[1], len(ex)


def _ptr(t):
    """Device pointer of a torch tensor (fp64, contiguous, on the GPU) or None."""
    if t is None:
        return None
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), \
        'expected a contiguous float64 CUDA/HIP tensor'
    return C.c_void_p(t.data_ptr())


class HipContext:
    """Thin object wrapper over the C-ABI; all tensors are torch float64 tensors on the context's device."""

    def __init__(self, n_atoms, box, device=0, stream=None, rank=0, world=1):
        import torch
        if not torch.cuda.is_available():
            raise HipError('no HIP device visible to torch: the HIP path has no CPU fallback')
        L = lib()
        self.n = int(n_atoms)
        self.device = int(device)
        self.torch_device = torch.device('cuda', self.device)
        torch.cuda.set_device(self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.torch_device).cuda_stream
        # box = None: a context without a periodic box (free-space pair forces and non-periodic terms only)
        b, bp = (None, None) if box is None else _hd(np.asarray(box, dtype=np.float64).reshape(3))
        h = C.c_void_p()
        _chk(L.amm_create(self.n, bp, self.device, C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.rank, self.world = rank, world
        self.has_comm = False
        if world > 1:
            _chk(L.amm_set_slice(self.h, rank, world))
        self._keep = []
        self._cmap_doubles = {}         # CMAP force id -> number of coefficients it was created with (amm_cmap_set_params reads as many)

    def close(self):
        """Release the context (and its RCCL communicator) NOW.  Idempotent.  Contexts still open when the interpreter exits are
        closed by an atexit hook, while the HIP runtime and RCCL are still whole: left to __del__ during interpreter
        finalisation, ncclCommDestroy can run after the runtime it needs has begun to shut down (the stuck RCCL worker of
        round 3)."""
        if getattr(self, 'h', None):
            _LIVE.discard(self)
            lib().amm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_globals(self, entry_point, fid, globals_):
        """New values of the globals of a text-driven force, in the program's order."""
        _chk(entry_point(self.h, fid, *_globals(globals_)))

    # ---- forces
    def pair_create(self, desc, q, sigma, eps, excl_pairs=None, skin=-1.0):
        q_, qp = _hd(q); s_, sp = _hd(sigma); e_, ep = _hd(eps)
        assert len(q_) == len(s_) == len(e_) == self.n
        ex = np.zeros((0, 2), np.int32) if excl_pairs is None else np.asarray(excl_pairs, dtype=np.int32).reshape(-1, 2)
        ex_, exp_ = _hi(ex)
        fid = C.c_int32(-1)
        _chk(lib().amm_pair_create(self.h, C.byref(desc), qp, sp, ep, exp_, len(ex_), float(skin), C.byref(fid)))
        return fid.value

    def pair_expr_create(self, desc, code, consts, globals_, p0, p1, p2, excl_pairs=None, skin=-1.0):
        """A generic pair force (family PAIR_EXPR): the program of expr.compile_pair, the values of its globals in the program's order
        and the three per-particle parameter slots, stored raw (None: all zero)."""
        slots = [None if p is None else _hd(p) for p in (p0, p1, p2)]
        assert all(s is None or len(s[0]) == self.n for s in slots)
        ex = np.zeros((0, 2), np.int32) if excl_pairs is None else np.asarray(excl_pairs, dtype=np.int32).reshape(-1, 2)
        ex_, exp_ = _hi(ex)
        fid = C.c_int32(-1)
        _chk(lib().amm_pair_expr_create(self.h, C.byref(desc), *_program(code, consts, globals_),
                                        *[None if s is None else s[1] for s in slots], exp_, len(ex_), float(skin), C.byref(fid)))
        return fid.value

    def pair_expr_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_pair_expr_set_globals, fid, globals_)

    def pair_expr_set_tables(self, fid, tables):
        """The tabulated functions of a generic pair force, in the force's function order: one (kind, nx, ny, lo, hi, doubles) each
        (atomsmm_amd/tables.py: device_table).  Again with new values of the same sizes: updateParametersInContext."""
        _chk(lib().amm_pair_expr_set_tables(self.h, fid, *self._table_arguments(tables)))

    def _table_arguments(self, tables):
        """(n_tables, kinds, dims, ranges, offsets, data, n_data) of amm_pair_expr_set_tables / amm_custom_gb_set_tables; the arrays
        stay alive in self._table_keep until the next call."""
        kinds = np.array([t[0] for t in tables], dtype=np.int32)
        dims = np.array([[t[1], t[2]] for t in tables], dtype=np.int32).reshape(-1)
        ranges = np.array([[t[3], t[4]] for t in tables], dtype=np.float64).reshape(-1)
        blocks = [np.ascontiguousarray(t[5], dtype=np.float64).reshape(-1) for t in tables]
        offsets = np.zeros(len(tables), dtype=np.int32)
        if tables:
            offsets[1:] = np.cumsum([len(b) for b in blocks])[:-1]
        data = np.concatenate(blocks) if blocks else np.zeros(0)
        k_, kp = _hi(kinds if len(tables) else [0])
        d_, dmp = _hi(dims if len(tables) else [0])
        r_, rp = _hd(ranges if len(tables) else [0.0])
        o_, op = _hi(offsets if len(tables) else [0])
        v_, vp = _hd(data if len(data) else [0.0])
        self._table_keep = (k_, d_, r_, o_, v_)
        return len(tables), kp, dmp, rp, op, vp, len(data)

    def pair_share_list(self, fid, host_fid):
        _chk(lib().amm_pair_share_list(self.h, fid, host_fid))

    def pair_set_params(self, fid, q, sigma, eps):
        q_, qp = _hd(q); s_, sp = _hd(sigma); e_, ep = _hd(eps)
        _chk(lib().amm_pair_set_params(self.h, fid, qp, sp, ep))

    def pair_energy_derivative(self, fid, pos, out):
        _chk(lib().amm_pair_energy_derivative(self.h, fid, _ptr(pos), _ptr(out)))

    def pair_energy_states(self, fid, pos, lambdas, out):
        """out[k] += energy of softcore force `fid` at lambda = lambdas[k] (device fp64 tensors of equal length, 1..MAX_STATES), energy
        only; the force's own lambda stays as it is."""
        assert lambdas.numel() == out.numel(), 'one output per lambda'
        _chk(lib().amm_pair_energy_states(self.h, fid, _ptr(pos), _ptr(lambdas), int(lambdas.numel()), _ptr(out)))

    def pair_set_scale(self, fid, value):
        _chk(lib().amm_pair_set_scale(self.h, fid, float(value)))

    def pair_set_lambda(self, fid, value):
        _chk(lib().amm_pair_set_lambda(self.h, fid, float(value)))

    def pair_set_lambda_dev(self, fid, scalars, index):
        """lambda of a softcore force = scalars[index] (device tensor of doubles) at every later launch; scalars = None: back to the
        number of the last pair_set_lambda."""
        ptr = None if scalars is None else C.c_void_p(scalars.data_ptr() + 8 * int(index))
        _chk(lib().amm_pair_set_lambda_dev(self.h, fid, ptr))

    def expr_eval_scalar(self, code, consts, scalars):
        """Run a scalar program (atomsmm_amd.expr.compile_scalar pieces, each closed by OUT dst): scalars[dst] <- value, in order; DEVG
        operands are entries of `scalars`."""
        c_, cp = _hi(code)
        k_, kp = _hd(consts if len(consts) else [0.0])
        _chk(lib().amm_expr_eval_scalar(self.h, cp, len(c_), kp, len(consts), _ptr(scalars), int(scalars.numel())))

    def bonded_create(self):
        fid = C.c_int32(-1)
        _chk(lib().amm_bonded_create(self.h, C.byref(fid)))
        return fid.value

    def bonded_add_terms(self, fid, kind, idx, params, periodic=False, desc=None):
        idx_, ip = _hi(np.asarray(idx).reshape(-1, ARITY[kind]))
        par_, pp = _hd(np.asarray(params, dtype=np.float64).reshape(-1, NPAR[kind]))
        assert len(idx_) == len(par_)
        _chk(lib().amm_bonded_add_terms(self.h, fid, kind, ip, pp, len(idx_), int(bool(periodic)),
                                        C.byref(desc) if desc is not None else None))

    def bonded_finalize(self, fid, sliced=False):
        _chk(lib().amm_bonded_finalize(self.h, fid))
        if sliced:
            _chk(lib().amm_bonded_set_sliced(self.h, fid, 1))

    def bonded_stats(self, fid):
        """dict(ncomp, max_comp, terms_ok, G, mol3_ok, mixed_ok, n_gterms, n_sc): the layouts amm_bonded_finalize built for the set."""
        out = (C.c_int64 * 8)()
        _chk(lib().amm_bonded_stats(self.h, fid, out))
        return dict(zip(('ncomp', 'max_comp', 'terms_ok', 'G', 'mol3_ok', 'mixed_ok', 'n_gterms', 'n_sc'), (int(v) for v in out)))

    def bonded_release(self, fid):
        """Free a bond-list set that has been replaced (its id is retired)."""
        _chk(lib().amm_bonded_release(self.h, fid))

    def term_expr_create(self, kind, code, consts, globals_, idx, params, periodic=False):
        """A generic term force (csrc/term_expr.hip): the program of expr.compile_term, the values of its globals in the program's
        order, `idx` (n_terms x 4, padded with -1) and `params` (n_params x n_terms: parameter-major)."""
        idx_, ixp = _hi(np.asarray(idx, dtype=np.int32).reshape(-1, 4))
        pp, n_params = _param_major(params, len(idx_), keep_rows=True)
        fid = C.c_int32(-1)
        _chk(lib().amm_term_expr_create(self.h, int(kind), *_program(code, consts, globals_), ixp, pp, len(idx_), n_params,
                                        int(bool(periodic)), C.byref(fid)))
        return fid.value

    def term_expr_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_term_expr_set_globals, fid, globals_)

    def term_expr_set_params(self, fid, params, n_terms):
        """All per-term values again (n_params x n_terms, parameter-major)."""
        pp, n_params = _param_major(params, int(n_terms), keep_rows=True)
        _chk(lib().amm_term_expr_set_params(self.h, fid, pp, int(n_terms), n_params))

    def term_expr_release(self, fid):
        """Free a term-expression force (its id is retired)."""
        _chk(lib().amm_term_expr_release(self.h, fid))

    def compound_create(self, n_slots, code, consts, globals_, var_kinds, var_slots, idx, params, periodic=False, groups=None):
        """A compound-bond force (csrc/compound.hip): the program and the variable table of expr.compile_compound -- var_kinds[k] one of
        CVAR_*, var_slots[k] up to four positions within the bond --, the values of the program's globals in its order, `idx`
        (n_bonds x n_slots particles, or groups) and `params` (n_params x n_bonds: parameter-major).  groups: None (the slots are
        particles), or (ptr, atoms, weights) -- the members and weights of every group, CSR (a CustomCentroidBondForce)."""
        idx_ = np.asarray(idx, dtype=np.int32).reshape(-1, int(n_slots))
        ix_, ixp = _hi(idx_ if idx_.size else [0])
        pp, n_params = _param_major(params, len(idx_), keep_rows=True)
        if groups is None:
            n_groups, gpp, gap, gwp = 0, None, None, None
        else:
            ptr_, gpp = _hi(groups[0])
            at_, gap = _hi(groups[1] if len(groups[1]) else [0])
            w_, gwp = _hd(groups[2] if len(groups[2]) else [0.0])
            n_groups = len(groups[0]) - 1
        fid = C.c_int32(-1)
        _chk(lib().amm_compound_create(self.h, int(n_slots), *_program(code, consts, globals_), *_var_table(var_kinds, var_slots), ixp, pp,
                                       len(idx_), n_params, int(bool(periodic)), gpp, gap, gwp, n_groups, C.byref(fid)))
        return fid.value

    def compound_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_compound_set_globals, fid, globals_)

    def compound_set_params(self, fid, params, n_bonds):
        """All per-bond values again (n_params x n_bonds, parameter-major)."""
        pp, n_params = _param_major(params, int(n_bonds), keep_rows=True)
        _chk(lib().amm_compound_set_params(self.h, fid, pp, int(n_bonds), n_params))

    def compound_set_weights(self, fid, weights):
        """All group weights again, in the order of the groups' members."""
        w_, wp = _hd(weights if len(weights) else [0.0])
        _chk(lib().amm_compound_set_weights(self.h, fid, wp, len(weights)))

    def compound_release(self, fid):
        """Free a compound-bond force (its id is retired)."""
        _chk(lib().amm_compound_release(self.h, fid))

    def gb_create(self, q, radius, scale, eps_in=1.0, eps_out=78.3, sa_energy=2.25936, rc=0.0):
        """A GBSAOBCForce in free space (csrc/gb.hip): charge, radius (nm) and scale of every atom, the solute and solvent dielectric,
        the surface-area energy (kJ/mol/nm^2) and the cutoff (rc <= 0: NoCutoff)."""
        q_, qp = _hd(q); r_, rp = _hd(radius); s_, sp = _hd(scale)
        assert len(q_) == len(r_) == len(s_) == self.n
        fid = C.c_int32(-1)
        _chk(lib().amm_gb_create(self.h, qp, rp, sp, float(eps_in), float(eps_out), float(sa_energy), float(rc), C.byref(fid)))
        return fid.value

    def gb_set_params(self, fid, q, radius, scale, eps_in=1.0, eps_out=78.3, sa_energy=2.25936, rc=0.0):
        """Everything again (updateParametersInContext), checked as at creation."""
        q_, qp = _hd(q); r_, rp = _hd(radius); s_, sp = _hd(scale)
        assert len(q_) == len(r_) == len(s_) == self.n
        _chk(lib().amm_gb_set_params(self.h, fid, qp, rp, sp, float(eps_in), float(eps_out), float(sa_energy), float(rc)))

    def gb_born_radii(self, fid, pos):
        """The Born radii at `pos` as a numpy array (runs the first pass; waits for the stream)."""
        out = np.zeros(self.n, dtype=np.float64)
        _chk(lib().amm_gb_born_radii(self.h, fid, _ptr(pos), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def gb_release(self, fid):
        """Free a generalized-Born force (its id is retired)."""
        _chk(lib().amm_gb_release(self.h, fid))

    def cmap_create(self, sizes, coeffs, map_of_term, idx, periodic=False):
        """A CMAPTorsionForce (csrc/cmap.hip): the grid size of every map, the bicubic coefficients of all maps concatenated
        (tables.cmap_coefficients: 16 per cell), the map of every term and its eight atoms (n_terms x 8)."""
        s_, sp = _hi(sizes if len(sizes) else [0])
        c_, cp = _hd(coeffs if len(coeffs) else [0.0])
        assert len(coeffs) == 0 or c_.size == 16 * int(sum(int(k) * int(k) for k in sizes))
        m_, mp = _hi(map_of_term if len(map_of_term) else [0])
        idx_ = np.asarray(idx, dtype=np.int32).reshape(-1, 8)
        assert len(idx_) == len(map_of_term)
        ix_, ixp = _hi(idx_ if idx_.size else [0])
        fid = C.c_int32(-1)
        _chk(lib().amm_cmap_create(self.h, len(sizes), sp, cp, mp, ixp, len(idx_), int(bool(periodic)), C.byref(fid)))
        self._cmap_doubles[fid.value] = len(coeffs)
        return fid.value

    def cmap_set_params(self, fid, coeffs, map_of_term, n_maps):
        """All coefficients and all map indices again (updateParametersInContext): same maps, sizes and terms."""
        c_, cp = _hd(coeffs if len(coeffs) else [0.0])
        m_, mp = _hi(map_of_term if len(map_of_term) else [0])
        made_with = self._cmap_doubles.get(fid)
        if made_with is not None and len(coeffs) != made_with:
            raise HipError('cmap_set_params: %d coefficients given, the force was created with %d' % (len(coeffs), made_with))
        _chk(lib().amm_cmap_set_params(self.h, fid, cp, mp, int(n_maps), len(map_of_term)))

    def cmap_release(self, fid):
        """Free a CMAP force (its id is retired)."""
        _chk(lib().amm_cmap_release(self.h, fid))

    def custom_gb_create(self, n_values, types, programs, globals_, params, excl_pairs=None, rc=0.0):
        """A CustomGBForce in free space (csrc/custom_gb.hip).  types: SingleParticle 0 / ParticlePair 1 / ParticlePairNoExclusions 2 of
        the n_values computed values, then of the energy terms; programs: their (code, consts), as expr.compile_custom_gb emits them;
        globals_: the values of the force's globals in its order; params: n_params x n, parameter-major; rc <= 0: NoCutoff."""
        types = [int(t) for t in types]
        assert len(types) == len(programs) and 0 <= int(n_values) <= len(types)
        code_ptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in programs])]).astype(np.int32)
        const_ptr = np.concatenate([[0], np.cumsum([len(k) for _, k in programs])]).astype(np.int32)
        code = np.concatenate([np.asarray(c, dtype=np.int32).reshape(-1) for c, _ in programs] + [np.zeros(0, np.int32)])
        consts = np.concatenate([np.asarray(k, dtype=np.float64).reshape(-1) for _, k in programs] + [np.zeros(0)])
        pp, n_params = _param_major(params, self.n)
        t_, tp = _hi(types if types else [0])
        c_, cp = _hi(code if len(code) else [0])
        cp_, cpp = _hi(code_ptr)
        k_, kp = _hd(consts if len(consts) else [0.0])
        kp_, kpp = _hi(const_ptr)
        fid = C.c_int32(-1)
        _chk(lib().amm_custom_gb_create(self.h, n_params, int(n_values), len(types) - int(n_values), tp, cp, cpp, kp, kpp, *_globals(globals_),
                                        pp, *_pairs(excl_pairs), float(rc), C.byref(fid)))
        return fid.value

    def custom_gb_set_params(self, fid, params):
        """All per-particle values again (n_params x n, parameter-major)."""
        pp, n_params = _param_major(params, self.n)
        _chk(lib().amm_custom_gb_set_params(self.h, fid, pp, n_params, self.n))

    def custom_gb_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_custom_gb_set_globals, fid, globals_)

    def custom_gb_set_tables(self, fid, tables):
        """The tabulated functions of such a force, in its function order: one (kind, nx, ny, lo, hi, doubles) each, as
        pair_expr_set_tables takes them."""
        _chk(lib().amm_custom_gb_set_tables(self.h, fid, *self._table_arguments(tables)))

    def custom_gb_values(self, fid, pos, n_values):
        """The computed values at `pos` as a numpy array [n_values][n] (runs the value passes; waits for the stream)."""
        out = np.zeros((max(int(n_values), 1), self.n), dtype=np.float64)
        _chk(lib().amm_custom_gb_values(self.h, fid, _ptr(pos), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:int(n_values)]

    def custom_gb_release(self, fid):
        """Free a custom generalized-Born force (its id is retired)."""
        _chk(lib().amm_custom_gb_release(self.h, fid))

    def hbond_create(self, code, consts, globals_, var_kinds, var_slots, donors, acceptors, donor_params, acceptor_params, excl_pairs=None,
                     rc=0.0, periodic=False):
        """A hydrogen-bond force (csrc/hbond.hip): the program and the variable table of expr.compile_hbond -- var_kinds[k] one of
        CVAR_DISTANCE / CVAR_ANGLE / CVAR_DIHEDRAL, var_slots[k] its slots of the pair (0 .. 2 = d1 d2 d3, 3 .. 5 = a1 a2 a3) --
        donors / acceptors: n x 3 atoms (-1: the slot is not there); donor_params / acceptor_params: n_params x n, parameter-major;
        excl_pairs: (donor, acceptor) indices; rc <= 0: NoCutoff; periodic: CutoffPeriodic."""
        dn = np.asarray(donors, dtype=np.int32).reshape(-1, 3)
        ac = np.asarray(acceptors, dtype=np.int32).reshape(-1, 3)
        dn_, dnp = _hi(dn if len(dn) else [0])
        ac_, acp = _hi(ac if len(ac) else [0])
        fid = C.c_int32(-1)
        _chk(lib().amm_hbond_create(self.h, *_program(code, consts, globals_), *_var_table(var_kinds, var_slots), dnp, len(dn), acp, len(ac),
                                    *_param_major(donor_params, len(dn)), *_param_major(acceptor_params, len(ac)), *_pairs(excl_pairs),
                                    float(rc), 1 if periodic else 0, C.byref(fid)))
        return fid.value

    def hbond_set_params(self, fid, donor_params, n_donors, acceptor_params, n_acceptors):
        """All per-donor and per-acceptor values again (n_params x n each, parameter-major)."""
        dpp, n_dpar = _param_major(donor_params, int(n_donors))
        app, n_apar = _param_major(acceptor_params, int(n_acceptors))
        _chk(lib().amm_hbond_set_params(self.h, fid, dpp, int(n_donors), n_dpar, app, int(n_acceptors), n_apar))

    def hbond_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_hbond_set_globals, fid, globals_)

    def hbond_stats(self, fid):
        """dict(scanned, survivors, launches, chunks): the ordered pairs one pass scans, those that passed the cutoff and the
        exclusions in the last evaluation, kernel launches so far, column chunks per donor row (waits for the stream)."""
        out = (C.c_int64 * 4)()
        _chk(lib().amm_hbond_stats(self.h, fid, out))
        return dict(scanned=int(out[0]), survivors=int(out[1]), launches=int(out[2]), chunks=int(out[3]))

    def hbond_release(self, fid):
        """Free a hydrogen-bond force (its id is retired)."""
        _chk(lib().amm_hbond_release(self.h, fid))

    def many_create(self, code, consts, globals_, var_kinds, var_slots, params, types, n_types, perm_table, excl_pairs=None, rc=0.0,
                    periodic=False, central=False):
        """A many-particle force over sets of three (csrc/manyparticle.hip): the program and the variable table of
        expr.compile_many_particle -- var_kinds[k] one of CVAR_*, var_slots[k] its slots 0 .. 2 = p1 p2 p3 -- params: n_params x n,
        parameter-major; types: the dense type index of every particle; perm_table: n_types^3 permutation codes (-1: skip;
        engine.many_particle_table); excl_pairs: pairs of particles; rc <= 0: NoCutoff; periodic: CutoffPeriodic; central:
        UniqueCentralParticle."""
        ty = np.asarray(types, dtype=np.int32).reshape(-1)
        t_, tp = _hi(ty if len(ty) else [0])
        m_, mp = _hi(np.asarray(perm_table, dtype=np.int32).reshape(-1))
        fid = C.c_int32(-1)
        _chk(lib().amm_many_create(self.h, *_program(code, consts, globals_), *_var_table(var_kinds, var_slots), len(ty),
                                   *_param_major(params, len(ty)), tp, int(n_types), mp, *_pairs(excl_pairs), float(rc), 1 if periodic else 0,
                                   1 if central else 0, C.byref(fid)))
        return fid.value

    def many_set_params(self, fid, params, types, n_types, perm_table):
        """All per-particle values (n_params x n, parameter-major), the types and the permutation table again."""
        ty = np.asarray(types, dtype=np.int32).reshape(-1)
        pp, n_params = _param_major(params, len(ty))
        t_, tp = _hi(ty if len(ty) else [0])
        m_, mp = _hi(np.asarray(perm_table, dtype=np.int32).reshape(-1))
        _chk(lib().amm_many_set_params(self.h, fid, pp, len(ty), n_params, tp, int(n_types), mp))

    def many_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_many_set_globals, fid, globals_)

    def many_stats(self, fid):
        """dict(particles, sets, launches, fullest, capacity): the evaluations of the text whose energy the last evaluation summed
        (SinglePermutation: the sets; UniqueCentralParticle: one per set and centre), kernel launches so far, the fullest neighbour
        row of the last evaluation and the capacity of a row (waits for the stream)."""
        out = (C.c_int64 * 5)()
        _chk(lib().amm_many_stats(self.h, fid, out))
        return dict(particles=int(out[0]), sets=int(out[1]), launches=int(out[2]), fullest=int(out[3]), capacity=int(out[4]))

    def many_release(self, fid):
        """Free a many-particle force (its id is retired)."""
        _chk(lib().amm_many_release(self.h, fid))

    def rmsd_create(self, particles, reference):
        """An RMSD force (csrc/rmsd.hip): the selected particles and the reference rows of THOSE particles, [len(particles)][3] in nm,
        in the list's order; the library centres them."""
        p_, pp = _hi(np.asarray(particles, dtype=np.int32).reshape(-1) if len(particles) else [0])
        r_, rp = _hd(np.asarray(reference, dtype=np.float64).reshape(-1, 3) if len(particles) else [0.0])
        fid = C.c_int32(-1)
        _chk(lib().amm_rmsd_create(self.h, pp, len(particles), rp, C.byref(fid)))
        return fid.value

    def rmsd_set_reference(self, fid, particles, reference):
        """New particles and / or a new reference, laid out as at creation; their number may change (waits for the stream)."""
        p_, pp = _hi(np.asarray(particles, dtype=np.int32).reshape(-1) if len(particles) else [0])
        r_, rp = _hd(np.asarray(reference, dtype=np.float64).reshape(-1, 3) if len(particles) else [0.0])
        _chk(lib().amm_rmsd_set_reference(self.h, fid, pp, len(particles), rp))

    def rmsd_stats(self, fid):
        """dict(particles, blocks, launches_per_eval, launches): the path the force takes (1 block: one launch; else three)."""
        out = (C.c_int64 * 4)()
        _chk(lib().amm_rmsd_stats(self.h, fid, out))
        return dict(particles=int(out[0]), blocks=int(out[1]), launches_per_eval=int(out[2]), launches=int(out[3]))

    def rmsd_release(self, fid):
        """Free an RMSD force (its id is retired)."""
        _chk(lib().amm_rmsd_release(self.h, fid))

    def gayberne_create(self, active, axes, par, ex_ptr, ex_col, ex_par, rev_ptr, rev_src, rc=0.0, rs=-1.0, periodic=False):
        """A Gay-Berne force (csrc/gayberne.hip).  active: the interacting particles, ascending; axes[k]: the x- and y-particle of
        active[k] (-1: none); par[k]: sigma, epsilon, sx, sy, sz, ex, ey, ez; ex_ptr / ex_col / ex_par: the exceptions as a CSR over
        active rows -- columns (active indices) ascending, (sigma, epsilon) per entry, every pair on both rows; rev_ptr / rev_src: per
        particle of the context the 2 * row + (0: x, 1: y) that name it, ascending.  rc = 0: NoCutoff; rs < 0: no switch."""
        n_act = len(active)
        a_, ap = _hi(np.asarray(active, dtype=np.int32).reshape(-1) if n_act else [0])
        x_, xp = _hi(np.asarray(axes, dtype=np.int32).reshape(-1) if n_act else [0])
        p_, pp = _hd(np.asarray(par, dtype=np.float64).reshape(-1) if n_act else [0.0])
        ep_, epp = _hi(np.asarray(ex_ptr, dtype=np.int32).reshape(-1))
        ec_, ecp = _hi(np.asarray(ex_col, dtype=np.int32).reshape(-1) if len(ex_col) else [0])
        ev_, evp = _hd(np.asarray(ex_par, dtype=np.float64).reshape(-1) if len(ex_col) else [0.0])
        rp_, rpp = _hi(np.asarray(rev_ptr, dtype=np.int32).reshape(-1))
        rs_, rsp = _hi(np.asarray(rev_src, dtype=np.int32).reshape(-1) if len(rev_src) else [0])
        fid = C.c_int32(-1)
        _chk(lib().amm_gayberne_create(self.h, ap, n_act, xp, pp, epp, ecp, evp, rpp, rsp, float(rc), float(rs), int(bool(periodic)), C.byref(fid)))
        return fid.value

    def gayberne_set_params(self, fid, par, ex_par):
        """New parameter rows and exception values, laid out as at creation; the counts must not change (waits for the stream)."""
        par = np.asarray(par, dtype=np.float64).reshape(-1, 8)
        ex_par = np.asarray(ex_par, dtype=np.float64).reshape(-1, 2)
        p_, pp = _hd(par.reshape(-1) if len(par) else [0.0])
        e_, ep = _hd(ex_par.reshape(-1) if len(ex_par) else [0.0])
        _chk(lib().amm_gayberne_set_params(self.h, fid, pp, len(par), ep, len(ex_par)))

    def gayberne_stats(self, fid):
        """dict(active, scanned, survivors, launches, chunks): interacting particles, ordered pairs one evaluation tests, those that
        passed the cutoff and the exceptions in the last evaluation (each pair counts from both sides), launches so far, chunks per row."""
        out = (C.c_int64 * 5)()
        _chk(lib().amm_gayberne_stats(self.h, fid, out))
        return dict(active=int(out[0]), scanned=int(out[1]), survivors=int(out[2]), launches=int(out[3]), chunks=int(out[4]))

    def gayberne_release(self, fid):
        """Free a Gay-Berne force (its id is retired)."""
        _chk(lib().amm_gayberne_release(self.h, fid))

    def drude_create(self, idx, par, pairs, thole, periodic=False):
        """A Drude force (csrc/drude.hip).  idx[k]: particle, particle1 .. particle4 of Drude particle k (-1: none); par[k]: charge,
        polarizability, aniso12, aniso34; pairs[p]: the two Drude entries of screened pair p; thole[p]: its Thole factor."""
        idx = np.asarray(idx, dtype=np.int32).reshape(-1, 5)
        par = np.asarray(par, dtype=np.float64).reshape(-1, 4)
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        thole = np.asarray(thole, dtype=np.float64).reshape(-1)
        assert len(idx) == len(par) and len(pairs) == len(thole)
        i_, ip_ = _hi(idx.reshape(-1) if len(idx) else [0])
        p_, pp = _hd(par.reshape(-1) if len(par) else [0.0])
        s_, sp = _hi(pairs.reshape(-1) if len(pairs) else [0])
        t_, tp = _hd(thole if len(thole) else [0.0])
        fid = C.c_int32(-1)
        _chk(lib().amm_drude_create(self.h, ip_, pp, len(idx), sp, tp, len(pairs), int(bool(periodic)), C.byref(fid)))
        return fid.value

    def drude_set_params(self, fid, idx, par, pairs, thole):
        """New charges, polarizabilities, anisotropies and Thole factors, laid out as at creation; no index may change (waits for the stream)."""
        idx = np.asarray(idx, dtype=np.int32).reshape(-1, 5)
        par = np.asarray(par, dtype=np.float64).reshape(-1, 4)
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        thole = np.asarray(thole, dtype=np.float64).reshape(-1)
        i_, ip_ = _hi(idx.reshape(-1) if len(idx) else [0])
        p_, pp = _hd(par.reshape(-1) if len(par) else [0.0])
        s_, sp = _hi(pairs.reshape(-1) if len(pairs) else [0])
        t_, tp = _hd(thole if len(thole) else [0.0])
        _chk(lib().amm_drude_set_params(self.h, fid, ip_, pp, len(idx), sp, tp, len(pairs)))

    def drude_release(self, fid):
        """Free a Drude force (its id is retired)."""
        _chk(lib().amm_drude_release(self.h, fid))

    def drude_step_define(self, pairs, dt, friction, kT, drude_friction, drude_kT, max_distance=0.0):
        """The step of a DrudeLangevinIntegrator for OP_DRUDE_STEP: pairs[k] = (Drude particle, parent); dt in ps, frictions in 1/ps,
        kT in kJ/mol, the hard wall in nm (0: none)."""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        s_, sp = _hi(pairs.reshape(-1) if len(pairs) else [0])
        sid = C.c_int32(-1)
        _chk(lib().amm_drude_step_define(self.h, sp, len(pairs), float(dt), float(friction), float(kT), float(drude_friction), float(drude_kT),
                                         float(max_distance), C.byref(sid)))
        return sid.value

    def cv_create(self, inner_ids, n_deriv, code, consts, globals_):
        """A CustomCVForce with any energy text (csrc/cv.hip): the ids of the inner forces in the order of the collective variables
        (bond-list sets or term-expression forces, members of no group, the caller's to release), the program of expr.compile_cv --
        its variables are the collective variables, then the n_deriv derivative parameters -- and the values of its globals."""
        i_, ip_ = _hi(inner_ids)
        fid = C.c_int32()
        _chk(lib().amm_cv_create(self.h, ip_, len(i_), int(n_deriv), *_program(code, consts, globals_), C.byref(fid)))
        return fid.value

    def cv_set_globals(self, fid, globals_):
        self._set_globals(lib().amm_cv_set_globals, fid, globals_)

    def cv_set_variables(self, fid, values):
        """Current values of the derivative parameters, in the order of addEnergyParameterDerivative."""
        v_, vp = _hd(values if len(values) else [0.0])
        _chk(lib().amm_cv_set_variables(self.h, fid, vp, len(values)))

    def cv_values(self, fid, pos, n_cv):
        """The collective variables at `pos` (evaluates the inner forces; waits for the stream)."""
        out = np.zeros(int(n_cv), dtype=np.float64)
        _chk(lib().amm_cv_values(self.h, fid, _ptr(pos), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def cv_energy_derivative(self, fid, pos, out):
        """dE/dp of every derivative parameter, added to the device tensor `out` (one double per parameter); no wait."""
        _chk(lib().amm_cv_energy_derivative(self.h, fid, _ptr(pos), _ptr(out)))

    def cv_release(self, fid):
        """Free a collective-variable force (its id is retired; the inner forces stay)."""
        _chk(lib().amm_cv_release(self.h, fid))

    def pme_create(self, alpha, grid, q, Kc=KC):
        """Reciprocal space of a PME / Ewald NonbondedForce (smooth PME, order 5) on a grid[0] x grid[1] x grid[2] mesh."""
        q_, qp = _hd(q)
        fid = C.c_int32(-1)
        _chk(lib().amm_pme_create(self.h, float(alpha), int(grid[0]), int(grid[1]), int(grid[2]), float(Kc), qp, C.byref(fid)))
        return fid.value

    def pme_set_charges(self, fid, q):
        q_, qp = _hd(q)
        _chk(lib().amm_pme_set_charges(self.h, fid, qp))

    def pme_set_sliced(self, fid, on=True):
        _chk(lib().amm_pme_set_sliced(self.h, fid, int(bool(on))))

    def constraints_set_tolerance(self, tolerance):
        _chk(lib().amm_constraints_set_tolerance(self.h, float(tolerance)))

    def expr_define(self, code, consts, globals_):
        eid = C.c_int32(-1)
        _chk(lib().amm_expr_define(self.h, *_program(code, consts, globals_), C.byref(eid)))
        return eid.value

    def constraints_create(self, pairs, distances, tolerance=1e-5):
        p_, pp = _hi(np.asarray(pairs).reshape(-1, 2))
        d_, dp_ = _hd(distances)
        assert len(p_) == len(d_)
        _chk(lib().amm_constraints_create(self.h, pp, dp_, len(d_), float(tolerance)))

    # --- the library's own RCCL communicator (csrc/comm.hip)
    @staticmethod
    def rccl_path():
        """The librccl that torch already carries in this process (one copy must serve both)."""
        import torch
        path = os.path.join(os.path.dirname(torch.__file__), 'lib', 'librccl.so')
        return path.encode() if os.path.exists(path) else None

    @classmethod
    def comm_unique_id(cls, library=None):
        """library: path of the RCCL to bind (default: the one torch carries; the error-path tests pass a stand-in)."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _chk(lib().amm_comm_unique_id(library.encode() if library else cls.rccl_path(), buf))
        return buf.raw

    def comm_init(self, id_bytes, library=None):
        if len(id_bytes) != COMM_ID_BYTES:
            raise ValueError('communicator id must be %d bytes' % COMM_ID_BYTES)
        _chk(lib().amm_comm_init(self.h, library.encode() if library else self.rccl_path(), bytes(id_bytes), self.rank, self.world))
        self.has_comm = True

    def comm_destroy(self):
        _chk(lib().amm_comm_destroy(self.h))
        self.has_comm = False

    def comm_allreduce(self, tensor):
        _chk(lib().amm_comm_allreduce(self.h, _ptr(tensor), tensor.numel()))

    def comm_stats(self):
        out = (C.c_int64 * 2)()
        _chk(lib().amm_comm_stats(self.h, out))
        return dict(calls=out[0], doubles=out[1])

    def run_stats(self):
        """What amm_run_ops fused so far: launches that carried the inner RESPA loop as an epilogue, evaluations without a gather launch."""
        out = (C.c_int64 * 4)()
        _chk(lib().amm_run_stats(self.h, out))
        return dict(epilogues=out[0], copies_current=out[1], state_exchanges=out[2], scheduled=out[3])

    def run_rule_stats(self):
        """Who made the scheduling decisions of run_stats()['scheduled']: the plain path and the six fusion rules of csrc/run_ops.hip
        (their sum is 'scheduled'), and how many evaluations were offered an epilogue plan (carried ones: run_stats()['epilogues'])."""
        out = (C.c_int64 * 8)()
        _chk(lib().amm_run_rule_stats(self.h, out))
        return dict(zip(RULE_NAMES, out))

    def bath_define(self, z, kT):
        bid = C.c_int32(-1)
        _chk(lib().amm_bath_define(self.h, float(z), float(kT), C.byref(bid)))
        return bid.value

    def stock_define(self, kind, dt, friction, kT):
        """One of OpenMM's stock integrators (STOCK_*) for OP_STOCK: dt in ps, friction in 1/ps, kT in kJ/mol."""
        sid = C.c_int32(-1)
        _chk(lib().amm_stock_define(self.h, int(kind), float(dt), float(friction), float(kT), C.byref(sid)))
        return sid.value

    def bath_define_nhl(self, h, z, kT, Q, friction, slot):
        bid = C.c_int32(-1)
        _chk(lib().amm_bath_define_nhl(self.h, float(h), float(z), float(kT), float(Q), float(friction), int(slot), C.byref(bid)))
        return bid.value

    def bath_define_sin(self, h, z, kT, Q2, friction, slot_v2):
        bid = C.c_int32(-1)
        _chk(lib().amm_bath_define_sin(self.h, float(h), float(z), float(kT), float(Q2), float(friction), int(slot_v2), C.byref(bid)))
        return bid.value

    def iso_define(self, on, LkT=0.0, Q1=0.0, slot_v1=-1):
        _chk(lib().amm_iso_define(self.h, int(bool(on)), float(LkT), float(Q1), int(slot_v1)))

    def regulated_define(self, on, alpha=1.0, an_kT=0.0):
        """Regulated mode: every MOVE op is x <- x + c tanh(alpha v/c) coef with c = sqrt(an_kT/m)."""
        _chk(lib().amm_regulated_define(self.h, int(bool(on)), float(alpha), float(an_kT)))

    def bath_define_regulated(self, kind, split, h, z, kT, Q, omega, friction, alpha, an, slot_v_eta):
        """A regulated Nose-Hoover-Langevin bath block (kind 3..6, include/atomsmm_hip.h) as one BATH op."""
        bid = C.c_int32(-1)
        _chk(lib().amm_bath_define_regulated(self.h, int(kind), int(bool(split)), float(h), float(z), float(kT), float(Q), float(omega),
                                             float(friction), float(alpha), float(an), int(slot_v_eta), C.byref(bid)))
        return bid.value

    def expr_seed(self, seed):
        _chk(lib().amm_expr_seed(self.h, int(seed) & (2 ** 64 - 1)))

    def expr_eval(self, code, consts, globals_, seed, counter, dst=None, total=None):
        """Per-DOF postfix program (atomsmm_amd.expr): dst <- values, total <- their sum (device tensors or None)."""
        _chk(lib().amm_expr_eval(self.h, *_program(code, consts, globals_), int(seed) & (2 ** 64 - 1),
                                 int(counter) & (2 ** 64 - 1), _ptr(dst), _ptr(total)))

    def force_eval(self, fid, pos, force, accumulate=False, energy=None):
        _chk(lib().amm_force_eval(self.h, fid, _ptr(pos), _ptr(force), int(bool(accumulate)), _ptr(energy)))

    # ---- energy minimisation (csrc/minimize.hip): the L-BFGS vectors of LocalEnergyMinimizer.minimize on the device
    def min_create(self, scalars, mass=None, memory=8, max_step=0.1, force_input=True):
        """A minimiser object.  scalars: 8 doubles on the device (include/atomsmm_hip.h: amm_min_create) -- evaluations add the
        energy to scalars[0]; mass: [n] or None; force_input: begin / advance are handed forces, not gradients.  The caller keeps
        both tensors alive until min_release."""
        assert scalars.numel() >= 8
        mid = C.c_int32(-1)
        _chk(lib().amm_min_create(self.h, int(memory), float(max_step), int(bool(force_input)), _ptr(mass), _ptr(scalars), C.byref(mid)))
        return mid.value

    def min_release(self, mid):
        _chk(lib().amm_min_release(self.h, mid))

    def min_begin(self, mid, x=None, g=None):
        """Start at (x, g); without arguments: clear the history and go back to steepest descent at the stored point."""
        _chk(lib().amm_min_begin(self.h, mid, _ptr(x), _ptr(g)))

    def min_advance(self, mid, x, g):
        _chk(lib().amm_min_advance(self.h, mid, _ptr(x), _ptr(g)))

    def min_trial(self, mid, alpha, x_out):
        _chk(lib().amm_min_trial(self.h, mid, float(alpha), _ptr(x_out)))

    def min_scalars(self, mid):
        """(E, g.d, g.g, max|g|, newest pair dropped, pairs in use, step factor of the last trial, largest |d_atom|^2); waits for the stream."""
        out = (C.c_double * 8)()
        _chk(lib().amm_min_scalars(self.h, mid, out))
        return list(out)

    def min_stats(self, mid):
        out = (C.c_int64 * 8)()
        _chk(lib().amm_min_stats(self.h, mid, out))
        return dict(pairs=out[0], trials=out[1], dropped=out[2], restarts=out[3], resets=out[4], in_use=out[5], memory=out[6])

    def min_read(self, mid, what, memory=None):
        """Inspection (tests): 'gram' -> (2m+1, 2m+1), 'delta' -> (2m+1,), 'direction' -> (n, 3) numpy arrays."""
        m = memory if memory is not None else self.min_stats(mid)['memory']
        nb = 2 * m + 1
        shape = {'gram': (nb, nb), 'delta': (nb,), 'direction': (self.n, 3)}[what]
        out = np.zeros(shape, dtype=np.float64)
        _chk(lib().amm_min_read(self.h, mid, ['gram', 'delta', 'direction'].index(what), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # ---- step primitives
    def kick(self, v, f, mass, coef, fsub=None, fadd=None):
        second = fsub if fsub is not None else fadd
        _chk(lib().amm_kick(self.h, _ptr(v), _ptr(f), _ptr(second), int(fadd is not None), _ptr(mass), float(coef)))

    def move(self, x, v, coef):
        _chk(lib().amm_move(self.h, _ptr(x), _ptr(v), float(coef)))

    def copy(self, dst, src):
        _chk(lib().amm_copy(self.h, _ptr(dst), _ptr(src)))

    def mvv(self, v, mass, out):
        _chk(lib().amm_mvv(self.h, _ptr(v), _ptr(mass), _ptr(out)))

    def bind_state(self, x, v, mass):
        self._keep += [x, v, mass]
        _chk(lib().amm_bind_state(self.h, _ptr(x), _ptr(v), _ptr(mass)))

    def bind_buffer(self, slot, buf):
        self._keep.append(buf)
        _chk(lib().amm_bind_buffer(self.h, slot, _ptr(buf)))

    def group_define(self, group, slot, force_ids):
        ids, p = _hi(np.asarray(force_ids, dtype=np.int32).reshape(-1))
        _chk(lib().amm_group_define(self.h, group, slot, p, len(ids)))

    def group_set_exchange(self, group, mode):
        _chk(lib().amm_group_set_exchange(self.h, int(group), int(mode)))

    def bind_exchange(self, tensor):
        """Exchange buffer of the all-gather mode: world * 2 * exchange_per() * 3 doubles, owned by the caller."""
        self._keep.append(tensor)
        _chk(lib().amm_bind_exchange(self.h, _ptr(tensor), tensor.numel()))

    def exchange_finish(self):
        _chk(lib().amm_exchange_finish(self.h))

    def run_ops(self, ops, repeat=1):
        arr = (Op * len(ops))(*ops)
        _chk(lib().amm_run_ops(self.h, arr, len(ops), int(repeat)))

    def run_ops_host_exchanges(self, ops, repeat, exchange):
        """amm_run_ops for several ranks whose collectives the HOST makes: runs the program to its end, calling `exchange()` -- which
        must all-gather the chunks of the exchange buffer and call exchange_finish -- whenever an exchanged evaluation waits for it
        (include/atomsmm_hip.h: amm_run_ops_from)."""
        arr = (Op * len(ops))(*ops)
        cursor = C.c_int64(0)
        total = len(ops) * int(repeat)
        while True:
            _chk(lib().amm_run_ops_from(self.h, arr, len(ops), int(repeat), C.byref(cursor)))
            nf = C.c_int32(0)
            _chk(lib().amm_exchange_pending(self.h, C.byref(nf)))
            if nf.value:
                exchange(nf.value)          # (also the exchange of the program's last op: one more call winds the program up)
            elif cursor.value >= total:
                return

    def set_outer_skin(self, skin_out):
        _chk(lib().amm_set_outer_skin(self.h, float(skin_out)))

    def set_option(self, name, value):
        """Tuning / test option of the context (include/atomsmm_hip.h: amm_set_option); set before the first evaluation."""
        _chk(lib().amm_set_option(self.h, name.encode(), float(value)))

    def positions_changed(self):
        """The bound position buffer was written outside the library (option 'positions_private')."""
        _chk(lib().amm_positions_changed(self.h))

    # ---- a box that changes (constant-pressure runs)
    def set_box(self, edges):
        """New box edges (nm) for every later launch; raises, and keeps the old box, when a pair cutoff exceeds half an edge."""
        b, bp = _hd(np.asarray(edges, dtype=np.float64).reshape(3))
        _chk(lib().amm_set_box(self.h, bp))

    def box_stats(self):
        out = (C.c_int64 * 4)()
        _chk(lib().amm_box_stats(self.h, out))
        return dict(changes=out[0], regrids=out[1], waits=out[2])

    def mol_define(self, molecules):
        """The molecules (a sequence of atom-index sequences, every atom exactly once) that mol_scale moves."""
        ptr = np.zeros(len(molecules) + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(m) for m in molecules])
        atoms = np.concatenate([np.asarray(m, dtype=np.int32).reshape(-1) for m in molecules]) if len(molecules) else np.zeros(0, np.int32)
        p_, pp = _hi(ptr)
        a_, ap = _hi(atoms if len(atoms) else np.zeros(1, np.int32))
        _chk(lib().amm_mol_define(self.h, pp, ap, len(molecules)))

    def mol_scale(self, x, scale, saved=None):
        """x <- x + (scale - 1) * centre of the atom's molecule, per axis; saved (or None) <- the old x, bit for bit."""
        s_, sp = _hd(np.asarray(scale, dtype=np.float64).reshape(3))
        _chk(lib().amm_mol_scale(self.h, _ptr(x), _ptr(saved), sp))

    # ---- virtual sites
    def vsite_define(self, sites, kinds, parents, weights):
        """Virtual sites: atom index and kind (VSITE_*) per site, parents [n_sites][3] (-1 pads a site of two parents), weights
        [n_sites][3]; replaces an earlier definition, no sites removes it."""
        n = len(sites)
        if n == 0:
            _chk(lib().amm_vsite_define(self.h, 0, None, None, None, None))
            return
        s_, sp = _hi(np.asarray(sites).reshape(n))
        k_, kp = _hi(np.asarray(kinds).reshape(n))
        p_, pp = _hi(np.asarray(parents).reshape(n, 3))
        w_, wp = _hd(np.asarray(weights, dtype=np.float64).reshape(n, 3))
        _chk(lib().amm_vsite_define(self.h, n, sp, kp, pp, wp))

    def vsite_place(self, x):
        """Sites <- their parents' positions in x (a no-op without sites)."""
        _chk(lib().amm_vsite_place(self.h, _ptr(x)))

    def vsite_spread(self, x, f):
        """The sites' rows of f go to their parents' (J^T f at x) and become 0 (a no-op without sites)."""
        _chk(lib().amm_vsite_spread(self.h, _ptr(x), _ptr(f)))

    def vsite_stats(self):
        out = (C.c_int64 * 4)()
        _chk(lib().amm_vsite_stats(self.h, out))
        return dict(places=out[0], spreads=out[1], launches=out[2], sites=out[3])

    def exchange_per(self):
        """Slots of the cell-sorted order per rank (whole molecules of three): chunk geometry of the exchange buffer."""
        per = C.c_int32(0)
        _chk(lib().amm_exchange_per(self.h, C.byref(per)))
        return per.value

    def set_fuse_inner(self, on=True):
        _chk(lib().amm_set_fuse_inner(self.h, int(bool(on))))

    def synchronize(self):
        _chk(lib().amm_synchronize(self.h))

    def check(self):
        _chk(lib().amm_check(self.h))

    def pair_stats(self, fid):
        st = PairStats()
        _chk(lib().amm_pair_get_stats(self.h, fid, C.byref(st)))
        return {name: getattr(st, name) for name, _ in PairStats._fields_}

    def pair_row_padding(self, fid):
        """(lane-trips executed, row entries) of the molecule-row traversal of this force; (0, 0) for per-atom rows."""
        out = (C.c_int64 * 2)()
        _chk(lib().amm_pair_row_padding(self.h, fid, out))
        return int(out[0]), int(out[1])

    def pair_guest_factor(self, fid):
        """(gfac, unit kernel taken) of the last fused pass force `fid` rode on: (Kc sign)_guest / (Kc sign)_host, and whether the
        launch took the kernel that leaves the product by a factor of exactly 1.0 out; (0.0, False) if it never rode along."""
        out = (C.c_double * 2)()
        _chk(lib().amm_pair_guest_factor(self.h, fid, out))
        return float(out[0]), bool(out[1])

    def pair_count_within(self, fid, pos, r_within):
        """Directed list entries of force `fid` with r < r_within at `pos` (fp64 count on the device; synchronises)."""
        n = C.c_int64()
        _chk(lib().amm_pair_count_within(self.h, fid, _ptr(pos), float(r_within), C.byref(n)))
        return n.value

    def profile_enable(self, on=True, only=None):
        _chk(lib().amm_profile_enable(self.h, -(int(only) + 1) if (on and only is not None) else int(bool(on))))

    def profile_read(self, fid):
        n = C.c_int64(); ms = C.c_double()
        _chk(lib().amm_profile_read(self.h, fid, C.byref(n), C.byref(ms)))
        return n.value, ms.value
