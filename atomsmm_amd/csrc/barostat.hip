// atomsmm_amd/csrc/barostat.hip -- molecule scaling of a Monte Carlo barostat move (gfx950).
//
// MonteCarloBarostat of OpenMM scales the centre of every molecule with the box and moves the molecule's atoms rigidly with it
// [OpenMM: ReferenceMonteCarloBarostat::applyBarostat].  Here the molecules are registered once (amm_mol_define, CSR) and one launch
// moves them (amm_mol_scale): the centre c of a molecule is the unweighted mean of its atoms' positions, summed in list order, and
// every atom moves by (scale - 1) c per axis.  Nothing is wrapped: the engine's arrays never are, and translating a centre by a
// lattice vector commutes with scaling box and centre together.
//
// Two code paths share the launch, chosen per block:
//   * molecules of at most AMM_CLUSTER_ATOMS atoms (waters, ions, a Lennard-Jones fluid): one lane per molecule, atoms in registers;
//   * longer ones (a solute, a chain): one wavefront per molecule -- lane l sums atoms l, l + 64, ... in order, a 64-wide xor-shuffle
//     tree adds the lanes' sums (a + b and b + a are the same bits, so every lane ends with the same centre), and the lanes then
//     stride over the atoms again to move them.
// Every atom belongs to exactly one molecule (amm_mol_define checks it), so every position is written once and by the lane that read
// it: the saved copy (the bits a rejected move restores) is written on the same pass.
#include "amm_ctx.h"

#include <algorithm>

struct MolArgs {
    int n_small, n_long, small_blocks;
    const int *ptr, *atoms, *small, *lng;
    double *x, *saved;
    double sm1[3];                 // scale - 1
};

__device__ __forceinline__ void mol_scale_small(const MolArgs &A, int t) {
    if (t >= A.n_small) return;
    const int m = A.small[t], b = A.ptr[m], cnt = A.ptr[m + 1] - b;
    double p[AMM_CLUSTER_ATOMS][3];
    int at[AMM_CLUSTER_ATOMS];
    double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < AMM_CLUSTER_ATOMS; ++a) {
        if (a < cnt) {
            const int i = A.atoms[b + a];
            at[a] = i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[a][k] = A.x[3 * (size_t)i + k];
                c[k] += p[a][k];
            }
        }
    }
    const double inv = 1.0 / (double)cnt;
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = A.sm1[k] * (c[k] * inv);
#pragma unroll
    for (int a = 0; a < AMM_CLUSTER_ATOMS; ++a) {
        if (a < cnt) {
            const size_t o = 3 * (size_t)at[a];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (A.saved) A.saved[o + k] = p[a][k];
                A.x[o + k] = p[a][k] + d[k];
            }
        }
    }
}

__device__ __forceinline__ void mol_scale_long(const MolArgs &A, int w, int lane) {
    if (w >= A.n_long) return;                     // (wave-uniform)
    const int m = A.lng[w], b = A.ptr[m], e = A.ptr[m + 1];
    double c[3] = {0.0, 0.0, 0.0};
    for (int j = b + lane; j < e; j += AMM_WAVE) {
        const size_t o = 3 * (size_t)A.atoms[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += A.x[o + k];
    }
#pragma unroll
    for (int off = AMM_WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += __shfl_xor(c[k], off, AMM_WAVE);
    }
    const double inv = 1.0 / (double)(e - b);
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = A.sm1[k] * (c[k] * inv);
    for (int j = b + lane; j < e; j += AMM_WAVE) {
        const size_t o = 3 * (size_t)A.atoms[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double old = A.x[o + k];
            if (A.saved) A.saved[o + k] = old;
            A.x[o + k] = old + d[k];
        }
    }
}

// blocks [0, small_blocks): 256 small molecules each; the blocks behind them: four long molecules each (one per wavefront)
__global__ void __launch_bounds__(256) k_mol_scale(MolArgs A) {
    const int blk = (int)blockIdx.x;
    if (blk < A.small_blocks) mol_scale_small(A, blk * 256 + (int)threadIdx.x);
    else mol_scale_long(A, (blk - A.small_blocks) * 4 + (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

int amm_mol_free(amm_ctx *ctx) {
    for (int **p : {&ctx->d_mol_ptr, &ctx->d_mol_atoms, &ctx->d_mol_small, &ctx->d_mol_long}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    ctx->n_mol = ctx->n_mol_small = ctx->n_mol_long = 0;
    return 0;
}

int amm_mol_define_impl(amm_ctx *ctx, const int32_t *h_ptr, const int32_t *h_atoms, int n_mol) {
    const int n = ctx->n;
    if (n_mol <= 0 || h_ptr[0] != 0 || h_ptr[n_mol] != n) {
        amm_set_error("amm_mol_define: the molecules must hold every atom exactly once (CSR: ptr[0] = 0, ptr[n_mol] = atoms of the context)");
        return 1;
    }
    std::vector<char> seen((size_t)n, 0);
    std::vector<int> small, lng;
    for (int m = 0; m < n_mol; ++m) {
        const int b = h_ptr[m], e = h_ptr[m + 1];
        if (e <= b || e > n) {
            amm_set_error("amm_mol_define: molecule " + std::to_string(m) + " is empty or its range is out of order");
            return 1;
        }
        for (int j = b; j < e; ++j) {
            const int i = h_atoms[j];
            if (i < 0 || i >= n || seen[i]) {
                amm_set_error("amm_mol_define: atom " + std::to_string(i) + " of molecule " + std::to_string(m) +
                              (i < 0 || i >= n ? " is out of range" : " appears twice") + " (every atom belongs to exactly one molecule)");
                return 1;
            }
            seen[i] = 1;
        }
        (e - b <= AMM_CLUSTER_ATOMS ? small : lng).push_back(m);
    }
    // (n entries, each a different atom in range: every atom exactly once)
    AMM_HIP(hipStreamSynchronize(ctx->stream));          // a launch that reads the old tables may still be queued
    amm_mol_free(ctx);
    auto up = [&](int **d, const int *h, size_t count) -> int {
        if (count == 0) return 0;
        AMM_HIP(hipMalloc(d, sizeof(int) * count));
        AMM_HIP(hipMemcpy(*d, h, sizeof(int) * count, hipMemcpyHostToDevice));
        return 0;
    };
    if (up(&ctx->d_mol_ptr, h_ptr, (size_t)n_mol + 1) || up(&ctx->d_mol_atoms, h_atoms, (size_t)n) || up(&ctx->d_mol_small, small.data(), small.size()) ||
        up(&ctx->d_mol_long, lng.data(), lng.size()))
        return 1;
    ctx->n_mol = n_mol;
    ctx->n_mol_small = (int)small.size();
    ctx->n_mol_long = (int)lng.size();
    return 0;
}

int amm_mol_scale_impl(amm_ctx *ctx, double *d_x, double *d_x_saved, const double scale[3]) {
    if (ctx->n_mol <= 0) {
        amm_set_error("amm_mol_scale: no molecules are defined (amm_mol_define)");
        return 1;
    }
    if (ctx->world > 1) {           // (as amm_set_box: the ranks' slices and exchanges are made for the box of creation)
        amm_set_error("amm_mol_scale: a context that is one rank of several keeps the box it was created with");
        return 1;
    }
    MolArgs A;
    A.n_small = ctx->n_mol_small;
    A.n_long = ctx->n_mol_long;
    A.small_blocks = (A.n_small + 255) / 256;
    A.ptr = ctx->d_mol_ptr;
    A.atoms = ctx->d_mol_atoms;
    A.small = ctx->d_mol_small;
    A.lng = ctx->d_mol_long;
    A.x = d_x;
    A.saved = d_x_saved;
    for (int k = 0; k < 3; ++k) A.sm1[k] = scale[k] - 1.0;
    const int blocks = A.small_blocks + (A.n_long + 3) / 4;
    hipLaunchKernelGGL(k_mol_scale, dim3(blocks), dim3(256), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    ctx->pos_epoch++;              // (as amm_positions_changed: the bound buffer, or any other, has moved)
    return 0;
}
