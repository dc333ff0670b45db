// atomsmm_amd/csrc/pair_args.h -- launch arguments of the per-atom-row traversals (pair.hip: k_pair_nlist, k_pair_tab, k_count_within;
// pair_expr.hip: k_pair_expr), passed to the kernels by value.
#pragma once
#include "amm_ctx.h"

struct PairArgs {
    int s_begin, s_end, lpa_shift, cap;
    const int *perm;
    const int *nl;
    const int *nnb;        // entries at the front of the row
    const int *nnb_total;  // if non-null: total entries; those beyond nnb[a] are stored from the back of the row
    const double4 *posq_s;
    const double2 *lj_s;
    double *force;     // original order [n][3]
    double *epart;     // per-block energy partials
    int accumulate;
    Box box;
    double *gforce;    // dual evaluation: force buffer of the guest force that shares this list (same particles)
    int gaccumulate;
    int sorted_out;    // exchange by all-gather: rows go to force[3 (s - s_begin)] (this rank's chunk of the exchange buffer)
    int gsame;         // the guest accumulates into the SAME rows as the host (fused FarNonbondedForce): one store of the sum
    const int *active;     // filtered lists: the rows that hold entries (slice-relative) ...
    const int *n_active;   // ... and their number (device); null: every row of the slice is walked
    const int *n_long;     // ... of which this many, filed from the front of `active`, are long rows; the others sit at the back
    int active_size;       //     of its active_size slots (amm_active_row)
    int long_shift;        // > 0: the long rows are walked with 1 << long_shift lanes each, before the others (k_pair_tab)
};
