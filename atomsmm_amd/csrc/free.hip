// atomsmm_amd/csrc/free.hip -- all-pairs pair forces in free space (gfx950, fp64, wave64): NoCutoff and CutoffNonPeriodic.
//
// What OpenMM does for a NonbondedForce / CustomNonbondedForce whose nonbondedMethod is NoCutoff or CutoffNonPeriodic
// (forces.py:278-283 maps both; systems.py:371-372, 850-851): every pair of atoms that is not excluded, at the distance the
// positions give -- no box, no minimum image, no neighbour list.  A vacuum solute or a droplet has no box to grid, and without a
// cutoff there is nothing for a list to prune: the kernel below walks ALL atoms for every row.
//
// Decomposition (owner-computes, no atomics, fixed order of summation -- two evaluations at the same positions give the same bits):
//   * a block of 256 threads owns 256 >> lpr_shift force rows; row i is summed by lpr = 1 << lpr_shift consecutive lanes
//     (1 .. 64, chosen on the host from n: free_lanes_per_row) whose partial sums meet in the __shfl_xor butterfly of k_pair_nlist;
//     lane 0 of the row stores it and honours `accumulate`.  Every pair is evaluated from both sides.
//   * the block stages tiles of AMM_FREE_TILE j atoms in LDS once and walks each for all of its rows.  Global loads of a tile are
//     coalesced and 16 B wide (the positions, [n][3] doubles, come in as a contiguous run of double2 and are re-laid from a
//     staging area; the (sigma/2, 2 sqrt(eps)) records are double2 already).  In LDS a tile is three arrays of double2 --
//     (x, y), (z, q), (sigma/2, 2 sqrt(eps)): 48 B per atom, 12 KiB per 256 atoms -- so that the lanes of a row read consecutive
//     16 B entries of each (ds_read_b128, conflict-free; rows that share a wavefront read the same entries: a broadcast).
//   * exclusions (the CSR a PairForce keeps) are never evaluated.  Each row knows the index range [emin, emax] of its excluded
//     partners (with itself); only tiles whose index range meets it look anything up, all others run without the test.
//   * arithmetic: amm_pair_math with the arguments k_pair_nlist gives it -- (Kc q_i) q_j, the sum of the half-sigmas, the product
//     of the 2 sqrt(eps) -- and the same cutoff predicate (r2 < rc2, with the guard r2 <= rc0^2); rc <= 0 is NoCutoff (rc2 = inf).
//   * energy: per-block partial sums (half of the doubly counted pairs), added in block order by k_reduce_add.
#include <cmath>
#include <cstdint>
#include <limits>

#include "amm_ctx.h"
#include "pair_math.h"

#define AMM_FREE_TILE 256
#define AMM_FREE_BLOCK 256

struct FreeArgs {
    int n, lpr_shift;
    int wide;                      // positions are 16-byte aligned: the tile's positions come in as double2
    const double *pos;             // [n][3]
    const double *q;               // [n]
    const double2 *lj;             // [n] (sigma/2, 2 sqrt(eps))
    const int *excl_ptr, *excl_idx;
    double *force;                 // [n][3]
    double *epart;                 // per-block energy partials
    int accumulate;
};

__device__ double amm_erfcx_table_dev_f[AMM_ERFCX_NI * AMM_ERFCX_NC];
static bool g_erfcx_uploaded_f[64] = {false};

template <int FAM, int CMODE, bool GUARD, bool EN>
__global__ void __launch_bounds__(AMM_FREE_BLOCK) k_pair_free(FreeArgs A, PairConsts c) {
    constexpr bool NEEDS_ERFC = (FAM == AMM_DAMPED);
    __shared__ double s_tab[NEEDS_ERFC ? AMM_ERFCX_NI * AMM_ERFCX_NC : 1];
    __shared__ __align__(16) double s_raw[3 * AMM_FREE_TILE];
    __shared__ double2 s_xy[AMM_FREE_TILE], s_zq[AMM_FREE_TILE], s_lj[AMM_FREE_TILE];
    const int tid = threadIdx.x;
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int rows_per_block = AMM_FREE_BLOCK >> A.lpr_shift;
    const int i = blockIdx.x * rows_per_block + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    if (NEEDS_ERFC) {
        for (int k = tid; k < AMM_ERFCX_NI * AMM_ERFCX_NC; k += AMM_FREE_BLOCK) s_tab[k] = amm_erfcx_table_dev_f[k];
    }
    double xi = 0.0, yi = 0.0, zi = 0.0, qi = 0.0, hsi = 0.0, sei = 0.0;
    int e0 = 0, e1 = 0, emin = 0x7fffffff, emax = -1;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        qi = c.Kc * A.q[i];
        const double2 li = A.lj[i];
        hsi = li.x;
        sei = li.y;
        e0 = A.excl_ptr[i];
        e1 = A.excl_ptr[i + 1];
        emin = emax = i;                    // (the pair j == i is skipped like an exclusion)
        for (int e = e0; e < e1; ++e) {
            const int j = A.excl_idx[e];
            emin = j < emin ? j : emin;
            emax = j > emax ? j : emax;
        }
    }
    const double guard2 = GUARD ? c.rc0 * c.rc0 : 0.0;
    double fx = 0.0, fy = 0.0, fz = 0.0, esum = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_FREE_TILE) {
        const int nt = (A.n - j0) < AMM_FREE_TILE ? (A.n - j0) : AMM_FREE_TILE;
        __syncthreads();                    // the previous tile has been walked by every row (and s_tab is written)
        {
            const int nd = 3 * nt;
            const double *src = A.pos + 3 * (size_t)j0;      // (j0 is a multiple of 256: as aligned as A.pos)
            if (A.wide) {
                const int nd2 = nd >> 1;
                for (int k = tid; k < nd2; k += AMM_FREE_BLOCK)
                    reinterpret_cast<double2 *>(s_raw)[k] = reinterpret_cast<const double2 *>(src)[k];
                if (tid == 0 && (nd & 1)) s_raw[nd - 1] = src[nd - 1];
            } else {
                for (int k = tid; k < nd; k += AMM_FREE_BLOCK) s_raw[k] = src[k];
            }
            if (tid < nt) s_lj[tid] = A.lj[j0 + tid];
        }
        __syncthreads();
        if (tid < nt) {
            s_xy[tid] = make_double2(s_raw[3 * tid], s_raw[3 * tid + 1]);
            s_zq[tid] = make_double2(s_raw[3 * tid + 2], A.q[j0 + tid]);
        }
        __syncthreads();
        if (!valid) continue;               // (no barrier is skipped: the three above are outside this test)
        // does this tile hold the row's own atom or one of its excluded partners?
        const bool check = emax >= j0 && emin < j0 + nt;
        for (int k = sub; k < nt; k += lpr) {
            const double2 xy = s_xy[k], zq = s_zq[k], lj = s_lj[k];
            bool ok = true;
            if (check) {
                const int j = j0 + k;
                ok = j != i;
                for (int e = e0; e < e1; ++e) ok = ok && (A.excl_idx[e] != j);
            }
            const double dx = xi - xy.x, dy = yi - xy.y, dz = zi - zq.x;
            const double r2 = dx * dx + dy * dy + dz * dz;
            bool pass = ok && (r2 < c.rc2);
            if (GUARD) pass = pass && (r2 <= guard2);            // step(rc0 - r)
            const double r2s = pass ? r2 : 1.0;
            double e, fr;
            amm_pair_math<FAM, CMODE, false, EN>(c, r2s, qi * zq.y, hsi + lj.x, sei * lj.y, e, fr, s_tab);
            fr = pass ? fr : 0.0;
            fx += fr * dx;
            fy += fr * dy;
            fz += fr * dz;
            if (EN) esum += pass ? e : 0.0;
        }
    }
    // combine the lpr partial sums of each row (fixed butterfly order -> deterministic)
    for (int off = lpr >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
    }
    if (valid && sub == 0) {
        double *f = A.force + 3 * (size_t)i;
        if (A.accumulate) {
            f[0] += fx;
            f[1] += fy;
            f[2] += fz;
        } else {
            f[0] = fx;
            f[1] = fy;
            f[2] = fz;
        }
    }
    if (EN) {
        __shared__ double red[AMM_FREE_BLOCK / 64];
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off);
        if ((tid & 63) == 0) red[tid >> 6] = esum;
        __syncthreads();
        if (tid == 0) A.epart[blockIdx.x] = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]);
    }
}

// DAMPED and NONBONDED carry no guard (as on the list path): two instantiations each, not four
template <int FAM, int CMODE>
static void launch_free_unguarded(dim3 grid, hipStream_t st, bool en, const FreeArgs &A, const PairConsts &c) {
    const dim3 block(AMM_FREE_BLOCK);
    if (en) hipLaunchKernelGGL((k_pair_free<FAM, CMODE, false, true>), grid, block, 0, st, A, c);
    else hipLaunchKernelGGL((k_pair_free<FAM, CMODE, false, false>), grid, block, 0, st, A, c);
}

template <int FAM, int CMODE>
static void launch_free(dim3 grid, hipStream_t st, bool guard, bool en, const FreeArgs &A, const PairConsts &c) {
    const dim3 block(AMM_FREE_BLOCK);
    if (guard) {
        if (en) hipLaunchKernelGGL((k_pair_free<FAM, CMODE, true, true>), grid, block, 0, st, A, c);
        else hipLaunchKernelGGL((k_pair_free<FAM, CMODE, true, false>), grid, block, 0, st, A, c);
    } else {
        if (en) hipLaunchKernelGGL((k_pair_free<FAM, CMODE, false, true>), grid, block, 0, st, A, c);
        else hipLaunchKernelGGL((k_pair_free<FAM, CMODE, false, false>), grid, block, 0, st, A, c);
    }
}

// Lanes per force row: the largest power of two <= 64 that keeps n * lanes within two blocks of 256 threads per CU of a
// 256-CU chip (131072 threads) -- a 33-atom solute gets whole wavefronts per row, a 12 000-atom droplet 8 lanes, 32 768 atoms 4.
int amm_free_lanes_per_row(int n) {
    int lpr = 64;
    while (lpr > 1 && (long)n * lpr > 131072L) lpr >>= 1;
    return lpr;
}

// Which descriptors k_pair_free has an instantiation for (amm_pair_create refuses the others).
int amm_free_supported(const amm_pair_desc &d, std::string &why) {
    if (d.flags & (AMM_GROUP_LJ | AMM_GROUP_Q)) {
        why = "interaction-group forces are not evaluated in free space";
        return 0;
    }
    if (d.flags & AMM_COULOMB_EWALD) {
        why = "Ewald sums need a periodic box";
        return 0;
    }
    switch (d.family) {
    case AMM_NONBONDED: return 1;
    case AMM_NEAR_NONE:
    case AMM_NEAR_SHIFT:
    case AMM_NEAR_FSWITCH:
    case AMM_DAMPED:
        if (!(d.rc > 0.0)) {
            why = "only the NONBONDED family is defined without a cutoff (rc <= 0)";
            return 0;
        }
        return 1;
    default:
        why = "the SOFTCORE and LJ_VIRIAL families are not evaluated in free space";
        return 0;
    }
}

int amm_free_eval_impl(amm_ctx *ctx, PairForce *pf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    hipStream_t st = ctx->stream;
    const int n = pf->n;
    if (!g_erfcx_uploaded_f[ctx->device & 63]) {
        AMM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(amm_erfcx_table_dev_f), amm_erfcx_table_host, sizeof(amm_erfcx_table_host)));
        g_erfcx_uploaded_f[ctx->device & 63] = true;
    }
    const int lpr = amm_free_lanes_per_row(n);
    int shift = 0;
    while ((1 << shift) < lpr) ++shift;
    const int rows_per_block = AMM_FREE_BLOCK >> shift;
    const int nblocks = (n + rows_per_block - 1) / rows_per_block;
    pf->lpa = lpr;
    const bool en = d_energy != nullptr;
    if (en && pf->n_epart < nblocks) {
        if (pf->d_epart) (void)hipFree(pf->d_epart);
        pf->d_epart = nullptr;
        AMM_HIP(hipMalloc(&pf->d_epart, sizeof(double) * nblocks));
        pf->n_epart = nblocks;
    }
    FreeArgs A;
    A.n = n;
    A.lpr_shift = shift;
    A.wide = ((uintptr_t)d_pos & 15) == 0 ? 1 : 0;
    A.pos = d_pos;
    A.q = pf->d_q;
    A.lj = pf->d_lj_s;
    A.excl_ptr = pf->d_excl_ptr;
    A.excl_idx = pf->d_excl_idx;
    A.force = d_force;
    A.epart = pf->d_epart;
    A.accumulate = accumulate;
    const PairConsts &c = pf->pc;
    const bool guard = (c.flags & AMM_GUARD_RC0) != 0;
    const dim3 grid(nblocks);
    switch (c.family) {
    case AMM_NEAR_NONE: launch_free<AMM_NEAR_NONE, 0>(grid, st, guard, en, A, c); break;
    case AMM_NEAR_SHIFT: launch_free<AMM_NEAR_SHIFT, 0>(grid, st, guard, en, A, c); break;
    case AMM_NEAR_FSWITCH: launch_free<AMM_NEAR_FSWITCH, 0>(grid, st, guard, en, A, c); break;
    case AMM_DAMPED:
        if (c.degree == 1) launch_free_unguarded<AMM_DAMPED, 1>(grid, st, en, A, c);
        else launch_free_unguarded<AMM_DAMPED, 0>(grid, st, en, A, c);
        break;
    case AMM_NONBONDED:
        if (c.cmode == 2) launch_free_unguarded<AMM_NONBONDED, 2>(grid, st, en, A, c);
        else launch_free_unguarded<AMM_NONBONDED, 0>(grid, st, en, A, c);
        break;
    default: amm_set_error("free-space pair force: no kernel for this family"); return 1;
    }
    AMM_HIP(hipGetLastError());
    pf->n_evals++;
    if (en) return amm_reduce_add(ctx, pf->d_epart, nblocks, 1.0, d_energy);
    return 0;
}
