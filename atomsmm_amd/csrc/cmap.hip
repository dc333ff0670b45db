// atomsmm_amd/csrc/cmap.hip -- CMAPTorsionForce (AMM_FORCE_CMAP): a term is a pair of dihedrals (phi over atoms a1..a4, psi over
// b1..b4) and its energy the value at (phi, psi) of a map tabulated on a size x size grid over [0, 2 pi)^2, interpolated by the
// tensor-product periodic cubic spline.  The spline is prepared on the host (atomsmm_amd/tables.py: cmap_coefficients) as 16
// coefficients per cell: E = sum_ij c[4 i + j] da^i db^j with da, db in [0, 1) the fractional positions within the cell.
//
// Takes over what OpenMM does for this class: per term the two dihedrals, the bicubic patch and its two partial derivatives, and
// -dE/dphi grad phi, -dE/dpsi grad psi on the eight atoms.  The geometry is that of the AMM_TERM_TORSION branch of k_term_expr
// (term_expr.hip): delta3 / cross3 / amm_min_image of bonded_terms.h, the dihedral convention and the four gradients of
// AMM_TORSION_PERIODIC.
//
// Two launches, no atomics, the pattern of k_term_expr / k_term_expr_gather: k_cmap evaluates one term per lane and parks the forces
// of its eight roles (24 doubles per term); k_cmap_gather, one lane per atom, adds the atom's (term, role) records in record order
// from a CSR built at creation -- an atom that a term names twice has two records -- and writes every row when it does not
// accumulate.  The energy goes through k_term_expr's fixed-order block reduction into per-block partials.  fp contraction is off and
// the energy instantiation computes the forces with the same operations as the force-only one: the same bits.
//
// Layout: the coefficients of all maps are concatenated, one contiguous row of 16 doubles (128 B, 128-byte aligned) per cell, cell
// (s, t) of a map at row offset + s + size * t; a small table holds (offset, size) per map.  A lane reads its row as eight 16-byte
// loads.  The cell index is reduced modulo the size before the read, so no position, however degenerate, indexes past a map.
// A force has hundreds to a few thousand terms: one wave per SIMD at the most, so the evaluation is bound by the launch and by the
// latency of three dependent reads (atoms, positions, coefficients), not by fp64 throughput.  DESIGN.md 3.CM has the resource figures.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "device_utils.h"

#define AMM_CMAP_BLOCK 256

struct CmapForce {
    int n_maps = 0, n_terms = 0, periodic = 0, n_blocks = 1;
    size_t n_cells = 0;                 // of all maps together
    int2 *d_map = nullptr;              // [n_maps] (row offset, size)
    double *d_coef = nullptr;           // [n_cells][16]
    int *d_map_of_term = nullptr;       // [n_terms]
    int *d_idx = nullptr;               // [n_terms][8] atoms: a1..a4, b1..b4
    double *d_park = nullptr;           // [n_terms][8][3] parked forces of the roles
    double *d_epart = nullptr;          // [n_blocks]
    int *d_ref_ptr = nullptr;           // [n + 1]: CSR of the (term, role) records of an atom ...
    int *d_rec_src = nullptr;           // ... each term * 8 + role, in that order
};

struct CmapArgs {
    int n_terms, periodic;
    const int *idx;
    const int *map_of_term;
    const int2 *map;
    const double *coef;
    const double *pos;
    double *park;
    double *epart;
    Box box;
};

// the dihedral of k_term_expr's torsion branch and its gradient on the four atoms
__device__ __forceinline__ double cmap_dihedral(const PosPlain &pos, const int *ix, const Box &box, int periodic, double *gi, double *gj,
                                                double *gk, double *gl) {
#pragma clang fp contract(off)
    double F[3], G[3], H[3], Av[3], Bv[3], BA[3];
    delta3(pos, ix[0], ix[1], box, periodic, F);
    delta3(pos, ix[1], ix[2], box, periodic, G);
    delta3(pos, ix[3], ix[2], box, periodic, H);
    cross3(F, G, Av);
    cross3(H, G, Bv);
    cross3(Bv, Av, BA);
    const double Gn = sqrt(dot3(G, G));
    const double angle = atan2(dot3(BA, G) / Gn, dot3(Av, Bv));
    const double A2 = dot3(Av, Av), B2 = dot3(Bv, Bv), FG = dot3(F, G), HG = dot3(H, G);
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        gi[x] = -Gn / A2 * Av[x];
        gl[x] = Gn / B2 * Bv[x];
        gj[x] = Gn / A2 * Av[x] + FG / (A2 * Gn) * Av[x] - HG / (B2 * Gn) * Bv[x];
        gk[x] = -Gn / B2 * Bv[x] - FG / (A2 * Gn) * Av[x] + HG / (B2 * Gn) * Bv[x];
    }
    return angle;
}

// an angle of (-pi, pi] as a cell index in [0, size) and the fractional position within the cell.  -1e-17 + 2 pi rounds to 2 pi and
// gives s == size with da == 0: cell 0 at its node, the same point.  Whatever u is (not a number included), s is inside the map.
__device__ __forceinline__ int cmap_cell(double angle, int size, double delta, double &da) {
#pragma clang fp contract(off)
    const double kTwoPi = 6.283185307179586476925287;
    if (angle < 0.0) angle += kTwoPi;
    const double u = angle / delta;
    int s = u >= 0.0 && u < 2147483647.0 ? (int)u : 0;
    da = u - (double)s;
    s %= size;
    return s;
}

template <bool EN>
__global__ void __launch_bounds__(AMM_CMAP_BLOCK) k_cmap(CmapArgs A) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    double e = 0.0;
    if (t < A.n_terms) {
        const double kTwoPi = 6.283185307179586476925287;
        int ix[8];
        {
            const int4 lo = reinterpret_cast<const int4 *>(A.idx)[2 * (size_t)t], hi = reinterpret_cast<const int4 *>(A.idx)[2 * (size_t)t + 1];
            ix[0] = lo.x; ix[1] = lo.y; ix[2] = lo.z; ix[3] = lo.w;
            ix[4] = hi.x; ix[5] = hi.y; ix[6] = hi.z; ix[7] = hi.w;
        }
        const int2 m = A.map[A.map_of_term[t]];        // (row offset, size)
        const PosPlain pos{A.pos};
        double g[8][3];
        const double phi = cmap_dihedral(pos, ix, A.box, A.periodic, g[0], g[1], g[2], g[3]);
        const double psi = cmap_dihedral(pos, ix + 4, A.box, A.periodic, g[4], g[5], g[6], g[7]);
        const int size = m.y;
        const double delta = kTwoPi / (double)size;
        double da, db;
        const int s = cmap_cell(phi, size, delta, da);
        const int tt = cmap_cell(psi, size, delta, db);
        const double2 *row = reinterpret_cast<const double2 *>(A.coef + ((size_t)m.x + (size_t)s + (size_t)size * (size_t)tt) * 16);
        double c[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double2 v = row[k];
            c[2 * k] = v.x;
            c[2 * k + 1] = v.y;
        }
        // nested Horner: the inner polynomials in db (value and derivative), then the outer one in da
        double r[4], d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r[i] = ((c[4 * i + 3] * db + c[4 * i + 2]) * db + c[4 * i + 1]) * db + c[4 * i];
            d[i] = (3.0 * c[4 * i + 3] * db + 2.0 * c[4 * i + 2]) * db + c[4 * i + 1];
        }
        e = ((r[3] * da + r[2]) * da + r[1]) * da + r[0];
        const double dEda = (3.0 * r[3] * da + 2.0 * r[2]) * da + r[1];
        const double dEdb = ((d[3] * da + d[2]) * da + d[1]) * da + d[0];
        const double dEdphi = dEda / delta, dEdpsi = dEdb / delta;
        double *out = A.park + (size_t)t * 24;
#pragma unroll
        for (int role = 0; role < 8; ++role) {
            const double de = role < 4 ? dEdphi : dEdpsi;
#pragma unroll
            for (int x = 0; x < 3; ++x) out[3 * role + x] = -(de * g[role][x]);
        }
    }
    if (EN) block_energy_store_256(e, A.epart);
}

// one lane per atom: its records, in record order (k_term_expr_gather's sum)
__global__ void __launch_bounds__(256) k_cmap_gather(int n, const int *__restrict__ ref_ptr, const int *__restrict__ rec_src,
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

int amm_cmap_eval_impl(amm_ctx *ctx, CmapForce *cm, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    if (cm->n_terms > 0) {
        CmapArgs A;
        A.n_terms = cm->n_terms;
        A.periodic = cm->periodic;
        A.idx = cm->d_idx;
        A.map_of_term = cm->d_map_of_term;
        A.map = cm->d_map;
        A.coef = cm->d_coef;
        A.pos = d_pos;
        A.park = cm->d_park;
        A.epart = cm->d_epart;
        A.box = ctx->box;
        if (d_energy) hipLaunchKernelGGL((k_cmap<true>), dim3(cm->n_blocks), dim3(AMM_CMAP_BLOCK), 0, ctx->stream, A);
        else hipLaunchKernelGGL((k_cmap<false>), dim3(cm->n_blocks), dim3(AMM_CMAP_BLOCK), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
    }
    // (a force without terms still writes its rows: it may be the first member of its group)
    hipLaunchKernelGGL(k_cmap_gather, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, ctx->stream, n, cm->d_ref_ptr, cm->d_rec_src, cm->d_park,
                       d_force, accumulate);
    AMM_HIP(hipGetLastError());
    if (d_energy && cm->n_terms > 0) return amm_reduce_add(ctx, cm->d_epart, cm->n_blocks, 1.0, d_energy);
    return 0;
}

// ---- host ----
static int cm_check_maps(const char *who, const int32_t *h_map_of_term, int n_terms, int n_maps) {
    for (int t = 0; t < n_terms; ++t)
        if (h_map_of_term[t] < 0 || h_map_of_term[t] >= n_maps) {
            amm_set_error(std::string(who) + ": term " + std::to_string(t) + " names map " + std::to_string(h_map_of_term[t]) + " (the force has " +
                          std::to_string(n_maps) + " maps)");
            return 1;
        }
    return 0;
}

int amm_cmap_create_impl(amm_ctx *ctx, int n_maps, const int32_t *h_sizes, const double *h_coeffs, const int32_t *h_map_of_term,
                         const int32_t *h_idx, int n_terms, int periodic, CmapForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_cmap_create: " + what);
        return 1;
    };
    const int n = ctx->n;
    if (n_maps < 0 || n_terms < 0) return fail("a negative count");
    if (periodic && !ctx->has_box) return fail("periodic torsions, but the context has no periodic box");
    if (ctx->world > 1) return fail("a CMAP force (AMM_FORCE_CMAP) runs on a single rank");
    if ((long long)n_terms * 8 > (long long)INT_MAX) return fail("too many (term, role) records for a 32-bit index");
    std::vector<int2> map(n_maps);
    size_t n_cells = 0;
    for (int m = 0; m < n_maps; ++m) {
        const int size = h_sizes[m];
        if (size < 2) return fail("map " + std::to_string(m) + " has size " + std::to_string(size) + " (a map needs at least 2 x 2 values)");
        if (size > 16384 || n_cells + (size_t)size * size > (size_t)INT_MAX / 16) return fail("the maps have too many cells for a 32-bit row index");
        map[m] = make_int2((int)n_cells, size);
        n_cells += (size_t)size * size;
    }
    if (cm_check_maps("amm_cmap_create", h_map_of_term, n_terms, n_maps)) return 1;
    for (size_t k = 0; k < (size_t)n_terms * 8; ++k)
        if (h_idx[k] < 0 || h_idx[k] >= n) return fail("atom index " + std::to_string(h_idx[k]) + " of term " + std::to_string(k / 8) + " is out of range");
    AMM_HIP(hipSetDevice(ctx->device));
    CmapForce *cm = new CmapForce();
    cm->n_maps = n_maps;
    cm->n_terms = n_terms;
    cm->periodic = periodic ? 1 : 0;
    cm->n_blocks = std::max(1, (n_terms + AMM_CMAP_BLOCK - 1) / AMM_CMAP_BLOCK);
    cm->n_cells = n_cells;
    // CSR of the records per atom: term order, then role
    std::vector<int> ptr(n + 1, 0), src((size_t)n_terms * 8);
    for (size_t k = 0; k < (size_t)n_terms * 8; ++k) ptr[h_idx[k] + 1]++;
    for (int i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    {
        std::vector<int> fill(ptr.begin(), ptr.end() - 1);
        for (size_t k = 0; k < (size_t)n_terms * 8; ++k) src[fill[h_idx[k]]++] = (int)k;
    }
    auto alloc = [&]() {
        if (amm_upload(&cm->d_map, map.data(), map.size())) return 1;
        if (amm_upload(&cm->d_coef, h_coeffs, n_cells * 16)) return 1;       // (hipMalloc aligns to 256 B: every row is 128-byte aligned)
        if (amm_upload(&cm->d_map_of_term, h_map_of_term, (size_t)n_terms)) return 1;
        if (amm_upload(&cm->d_idx, h_idx, (size_t)n_terms * 8)) return 1;
        if (amm_upload(&cm->d_ref_ptr, ptr.data(), ptr.size())) return 1;
        if (amm_upload(&cm->d_rec_src, src.data(), src.size())) return 1;
        const size_t park = std::max<size_t>((size_t)n_terms * 24, 1);
        AMM_HIP(hipMalloc(&cm->d_park, sizeof(double) * park));
        AMM_HIP(hipMemset(cm->d_park, 0, sizeof(double) * park));
        AMM_HIP(hipMalloc(&cm->d_epart, sizeof(double) * cm->n_blocks));
        return 0;
    };
    if (alloc()) {
        amm_cmap_free(cm);
        return 1;
    }
    *out = cm;
    return 0;
}

int amm_cmap_set_params_impl(amm_ctx *ctx, CmapForce *cm, const double *h_coeffs, const int32_t *h_map_of_term, int n_maps, int n_terms) {
    if (n_maps != cm->n_maps || n_terms != cm->n_terms) {
        amm_set_error("amm_cmap_set_params: the force has " + std::to_string(cm->n_maps) + " maps and " + std::to_string(cm->n_terms) + " terms, " +
                      std::to_string(n_maps) + " and " + std::to_string(n_terms) + " given");
        return 1;
    }
    if ((cm->n_cells > 0 && !h_coeffs) || (n_terms > 0 && !h_map_of_term)) {
        amm_set_error("amm_cmap_set_params: null argument");
        return 1;
    }
    if (cm_check_maps("amm_cmap_set_params", h_map_of_term, n_terms, n_maps)) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));     // ordered after any kernel already queued on the stream that reads the old values
    if (cm->n_cells) AMM_HIP(hipMemcpy(cm->d_coef, h_coeffs, sizeof(double) * 16 * cm->n_cells, hipMemcpyHostToDevice));
    if (n_terms) AMM_HIP(hipMemcpy(cm->d_map_of_term, h_map_of_term, sizeof(int) * n_terms, hipMemcpyHostToDevice));
    return 0;
}

void amm_cmap_free(CmapForce *cm) {
    if (!cm) return;
    for (void *p : {(void *)cm->d_map, (void *)cm->d_coef, (void *)cm->d_map_of_term, (void *)cm->d_idx, (void *)cm->d_park, (void *)cm->d_epart,
                    (void *)cm->d_ref_ptr, (void *)cm->d_rec_src})
        if (p) (void)hipFree(p);
    delete cm;
}
