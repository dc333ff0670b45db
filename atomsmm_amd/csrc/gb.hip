// atomsmm_amd/csrc/gb.hip -- GBSAOBCForce: generalized-Born implicit solvent (OBC2) with a surface-area term, for free-space
// systems (gfx950, fp64, wave64).  Type AMM_FORCE_GB.
//
// The definition (units nm, kJ/mol, e; include/atomsmm_hip.h: amm_gb_create):
//   rho_i = R_i - 0.009, s_j = S_j rho_j;  a pair (i, j), i != j, takes part when there is no cutoff or r^2 < rc^2
//   I_i = 1/2 sum_j h(r_ij; rho_i, s_j) over the pairs that take part and have rho_i < r + s_j, with
//     L = 1 / max(rho_i, |r - s_j|), U = 1 / (r + s_j)
//     h = L - U + r (U^2 - L^2)/4 + ln(U/L)/(2 r) + s_j^2 (L^2 - U^2)/(4 r)  [+ 2 (1/rho_i - L) when rho_i < s_j - r]
//   Psi = I rho,  B = 1 / (1/rho - tanh(Psi - 0.8 Psi^2 + 4.85 Psi^3)/R)
//   E = -1/2 Kc (1/eps_in - 1/eps_out) sum_{i,j} q_i q_j / f_ij + 4 pi sa sum_i (R_i + 0.14)^2 (R_i/B_i)^6,
//     f_ij = sqrt(r^2 + B_i B_j exp(-r^2/(4 B_i B_j))), the double sum over the ordered pairs that take part and every i = j.
//
// Decomposition: that of free.hip -- a block of 256 threads owns 256 >> lpr_shift rows, a row is summed by 1 .. 64 consecutive lanes
// that meet in a __shfl_xor butterfly, the j atoms come through LDS in tiles of 256 staged with coalesced 16-byte loads, every pair
// is evaluated from both sides, no atomics, a fixed order of summation.  Three launches, each needing the completed sums of the one
// before:
//   1. k_gb_born:  tile record (x, y, z, s_j).  Row i sums h; its lane 0 finishes Psi, the tanh, B_i and dB_i/dI_i and stores both.
//   2. k_gb_pair:  tile record (x, y, z, q, B_j, 1/B_j).  Row i sums its energy, the force -dE_pol/dx_i at fixed Born radii, and
//                  dE_pol/dB_i (row-local: f_ij is symmetric in B_i B_j).  The finish adds the diagonal term and the surface term,
//                  stores g_i = dE/dI_i = (dE/dB_i) dB_i/dI_i and parks the row's force.  Energy: per-block partials, added in block
//                  order by amm_reduce_add; the instantiation without energy serves force-only calls.
//   3. k_gb_chain: tile record (x, y, z, rho_j, s_j, g_j).  Row k gathers both roles of atom k in one walk: g_k dh(r; rho_k, s_j)/dx_k
//                  (k owns the integral) and g_j dh(r; rho_j, s_k)/dx_k (k is the sphere in j's integral), adds the parked row of
//                  pass 2 and stores once, honouring `accumulate`.
// dh/dr: the terms through L and U cancel (dh/dU = 0 at U = 1/(r + s); dh/dL = 0 where L = 1/|r - s| and the engulfed term is
// counted, and L does not move where the max picks rho), which leaves dh/dr = (U^2 - L^2)(1 + s^2/r^2)/4 - ln(U/L)/(2 r^2).
// The branches of h (the pair does not count, the max picks rho, atom i lies inside j's scaled sphere) differ from lane to lane: they
// are selects on values, and a pair that does not take part is evaluated at r = 1 and discarded.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "amm_ctx.h"

#define AMM_GB_TILE 256
#define AMM_GB_BLOCK 256
#define AMM_GB_OFFSET 0.009
#define AMM_GB_PROBE 0.14
#define AMM_GB_ALPHA 1.0
#define AMM_GB_BETA 0.8
#define AMM_GB_GAMMA 4.85

struct GbForce {
    int n = 0;
    double pre = 0;                // Kc (1/eps_in - 1/eps_out)
    double rc2 = 0;                // rc^2, or +inf without a cutoff
    double *d_q = nullptr, *d_rho = nullptr, *d_s = nullptr, *d_R = nullptr;
    double *d_sa = nullptr;        // 4 pi sa (R + 0.14)^2 R^6: the surface energy of atom i is d_sa[i] / B_i^6
    double *d_B = nullptr, *d_dBdI = nullptr, *d_g = nullptr;
    double *d_fdir = nullptr;      // [n][3] rows of pass 2, read by pass 3
    double *d_epart = nullptr;
    int n_epart = 0;
    int64_t n_evals = 0;
};

struct GbArgs {
    int n, lpr_shift;
    int wide;                      // positions are 16-byte aligned: the tile's positions come in as double2
    int accumulate;
    const double *pos;             // [n][3]
    const double *q, *rho, *s, *R, *sa;
    double *B, *dBdI, *g, *fdir;
    double *force;                 // [n][3]
    double *epart;                 // per-block energy partials
    double rc2, pre;
};

// the positions of atoms j0 .. j0 + nt into s_raw as they lie in memory (coalesced; j0 is a multiple of 256: as aligned as pos)
__device__ __forceinline__ void gb_stage_raw(const GbArgs &A, int j0, int nt, double *s_raw, int tid) {
    const int nd = 3 * nt;
    const double *src = A.pos + 3 * (size_t)j0;
    if (A.wide) {
        const int nd2 = nd >> 1;
        for (int k = tid; k < nd2; k += AMM_GB_BLOCK) reinterpret_cast<double2 *>(s_raw)[k] = reinterpret_cast<const double2 *>(src)[k];
        if (tid == 0 && (nd & 1)) s_raw[nd - 1] = src[nd - 1];
    } else {
        for (int k = tid; k < nd; k += AMM_GB_BLOCK) s_raw[k] = src[k];
    }
}

// fp64 divisions are long sequences (scale, reciprocal estimate, refinement, fix-up): each pair takes ONE, of the product of
// everything it divides by, and the single reciprocals are that times the other factors (all of them between 1e-3 and 1e2 here).

// h(r; rho, s) of a pair with rho < r + s (the caller discards the others: every value here is finite for them too); inv_rho = 1/rho
__device__ __forceinline__ double gb_h(double r, double rho, double inv_rho, double s) {
    const double p = r + s;
    const double m = fmax(rho, fabs(r - s));
    const double inv = 1.0 / (r * p * m);
    const double U = inv * (r * m), L = inv * (r * p), inv_r = inv * (p * m);
    const double dl = L * L - U * U;
    const double h = L - U - 0.25 * r * dl + 0.5 * inv_r * log(U * m) + 0.25 * s * s * inv_r * dl;
    return h + ((rho < s - r) ? 2.0 * (inv_rho - L) : 0.0);
}

// (dh/dr) / r of such a pair from U = 1/(r + s), m = max(rho, |r - s|) and L = 1/m
__device__ __forceinline__ double gb_dh_over_r(double U, double m, double L, double s, double inv_r) {
    const double inv_r2 = inv_r * inv_r;
    return (0.25 * (U * U - L * L) * (1.0 + s * s * inv_r2) - 0.5 * inv_r2 * log(U * m)) * inv_r;
}

__global__ void __launch_bounds__(AMM_GB_BLOCK) k_gb_born(GbArgs A) {
    __shared__ __align__(16) double s_raw[3 * AMM_GB_TILE];
    __shared__ double2 s_xy[AMM_GB_TILE], s_zs[AMM_GB_TILE];
    const int tid = threadIdx.x;
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_GB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    double xi = 0.0, yi = 0.0, zi = 0.0, rho = 1.0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        rho = A.rho[i];
    }
    const double inv_rho = 1.0 / rho;
    double sum = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_GB_TILE) {
        const int nt = (A.n - j0) < AMM_GB_TILE ? (A.n - j0) : AMM_GB_TILE;
        __syncthreads();                    // the previous tile has been walked by every row
        gb_stage_raw(A, j0, nt, s_raw, tid);
        __syncthreads();
        if (tid < nt) {
            s_xy[tid] = make_double2(s_raw[3 * tid], s_raw[3 * tid + 1]);
            s_zs[tid] = make_double2(s_raw[3 * tid + 2], A.s[j0 + tid]);
        }
        __syncthreads();
        if (!valid) continue;               // (no barrier is skipped: the three above are outside this test)
        for (int k = sub; k < nt; k += lpr) {
            const double2 xy = s_xy[k], zs = s_zs[k];
            const double dx = xi - xy.x, dy = yi - xy.y, dz = zi - zs.x;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const bool part = (j0 + k != i) && (r2 < A.rc2);
            const double r = sqrt(part ? r2 : 1.0);
            const double h = gb_h(r, rho, inv_rho, zs.y);
            sum += (part && rho < r + zs.y) ? h : 0.0;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (valid && sub == 0) {
        const double R = A.R[i];
        const double psi = 0.5 * sum * rho;
        const double t = tanh(AMM_GB_ALPHA * psi - AMM_GB_BETA * psi * psi + AMM_GB_GAMMA * psi * psi * psi);
        const double B = 1.0 / (inv_rho - t / R);
        A.B[i] = B;
        A.dBdI[i] = B * B * (1.0 - t * t) * (AMM_GB_ALPHA - 2.0 * AMM_GB_BETA * psi + 3.0 * AMM_GB_GAMMA * psi * psi) * rho / R;
    }
}

template <bool EN>
__global__ void __launch_bounds__(AMM_GB_BLOCK) k_gb_pair(GbArgs A) {
    __shared__ __align__(16) double s_raw[3 * AMM_GB_TILE];
    __shared__ double2 s_xy[AMM_GB_TILE], s_zq[AMM_GB_TILE];
    __shared__ double2 s_B[AMM_GB_TILE];           // (B_j, 1 / B_j)
    const int tid = threadIdx.x;
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_GB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    double xi = 0.0, yi = 0.0, zi = 0.0, qi = 0.0, Bi = 1.0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        qi = A.pre * A.q[i];
        Bi = A.B[i];
    }
    const double inv_Bi = 1.0 / Bi;
    double fx = 0.0, fy = 0.0, fz = 0.0, dEdB = 0.0, esum = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_GB_TILE) {
        const int nt = (A.n - j0) < AMM_GB_TILE ? (A.n - j0) : AMM_GB_TILE;
        __syncthreads();
        gb_stage_raw(A, j0, nt, s_raw, tid);
        __syncthreads();
        if (tid < nt) {
            s_xy[tid] = make_double2(s_raw[3 * tid], s_raw[3 * tid + 1]);
            s_zq[tid] = make_double2(s_raw[3 * tid + 2], A.q[j0 + tid]);
            const double Bj = A.B[j0 + tid];
            s_B[tid] = make_double2(Bj, 1.0 / Bj);
        }
        __syncthreads();
        if (!valid) continue;
        for (int k = sub; k < nt; k += lpr) {
            const double2 xy = s_xy[k], zq = s_zq[k];
            const double2 bj = s_B[k];
            const double Bj = bj.x;
            const double dx = xi - xy.x, dy = yi - xy.y, dz = zi - zq.x;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const bool part = (j0 + k != i) && (r2 < A.rc2);
            const double r2s = part ? r2 : 1.0;
            const double D = Bi * Bj;
            const double a = 0.25 * r2s * (inv_Bi * bj.y);      // r^2 / (4 B_i B_j)
            const double ex = exp(-a);
            const double inv_f = rsqrt(r2s + D * ex);
            const double qq = part ? qi * zq.y : 0.0;          // Kc (1/eps_in - 1/eps_out) q_i q_j, or nothing
            const double w = qq * inv_f * inv_f * inv_f;
            const double fr = -w * (1.0 - 0.25 * ex);
            fx += fr * dx;
            fy += fr * dy;
            fz += fr * dz;
            dEdB += 0.5 * w * ex * (1.0 + a) * Bj;
            if (EN) esum += -0.5 * qq * inv_f;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
        dEdB += __shfl_xor(dEdB, off);
    }
    if (valid && sub == 0) {
        const double inv_B = inv_Bi;
        const double self = 0.5 * qi * A.q[i] * inv_B;         // the diagonal term is -self
        const double ib2 = inv_B * inv_B;
        const double esa = A.sa[i] * ib2 * ib2 * ib2;
        A.g[i] = (dEdB + self * inv_B - 6.0 * esa * inv_B) * A.dBdI[i];
        double *f = A.fdir + 3 * (size_t)i;
        f[0] = fx;
        f[1] = fy;
        f[2] = fz;
        if (EN) esum += esa - self;
    }
    if (EN) {
        __shared__ double red[AMM_GB_BLOCK / 64];
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off);
        if ((tid & 63) == 0) red[tid >> 6] = esum;
        __syncthreads();
        if (tid == 0) A.epart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

__global__ void __launch_bounds__(AMM_GB_BLOCK) k_gb_chain(GbArgs A) {
    __shared__ __align__(16) double s_raw[3 * AMM_GB_TILE];
    __shared__ double2 s_xy[AMM_GB_TILE], s_zr[AMM_GB_TILE], s_sg[AMM_GB_TILE];
    const int tid = threadIdx.x;
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_GB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    double xi = 0.0, yi = 0.0, zi = 0.0, rho_i = 1.0, s_i = 0.0, g_i = 0.0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        rho_i = A.rho[i];
        s_i = A.s[i];
        g_i = A.g[i];
    }
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_GB_TILE) {
        const int nt = (A.n - j0) < AMM_GB_TILE ? (A.n - j0) : AMM_GB_TILE;
        __syncthreads();
        gb_stage_raw(A, j0, nt, s_raw, tid);
        __syncthreads();
        if (tid < nt) {
            s_xy[tid] = make_double2(s_raw[3 * tid], s_raw[3 * tid + 1]);
            s_zr[tid] = make_double2(s_raw[3 * tid + 2], A.rho[j0 + tid]);
            s_sg[tid] = make_double2(A.s[j0 + tid], A.g[j0 + tid]);
        }
        __syncthreads();
        if (!valid) continue;
        for (int k = sub; k < nt; k += lpr) {
            const double2 xy = s_xy[k], zr = s_zr[k], sg = s_sg[k];
            const double dx = xi - xy.x, dy = yi - xy.y, dz = zi - zr.x;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const bool part = (j0 + k != i) && (r2 < A.rc2);
            const double r = sqrt(part ? r2 : 1.0);
            const double pa = r + sg.x, ma = fmax(rho_i, fabs(r - sg.x));       // atom i owns the integral, j is the sphere
            const double pb = r + s_i, mb = fmax(zr.y, fabs(r - s_i));          // atom j owns the integral, i is the sphere
            const double wa = pa * ma, wb = pb * mb;
            const double inv = 1.0 / (r * wa * wb);
            const double inv_r = inv * (wa * wb);
            const double ia = inv * (r * wb), ib = inv * (r * wa);              // 1 / (pa ma), 1 / (pb mb)
            const double own = gb_dh_over_r(ia * ma, ma, ia * pa, sg.x, inv_r);
            const double sph = gb_dh_over_r(ib * mb, mb, ib * pb, s_i, inv_r);
            const double c_own = (part && rho_i < r + sg.x) ? g_i : 0.0;
            const double c_sph = (part && zr.y < r + s_i) ? sg.y : 0.0;
            const double fr = -0.5 * (c_own * own + c_sph * sph);
            fx += fr * dx;
            fy += fr * dy;
            fz += fr * dz;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
    }
    if (valid && sub == 0) {
        const double *d = A.fdir + 3 * (size_t)i;
        fx += d[0];
        fy += d[1];
        fz += d[2];
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
}

static int gb_check(const char *who, int n, const double *h_q, const double *h_radius, const double *h_scale, double eps_in, double eps_out,
                    double sa_energy) {
    auto fail = [&](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what);
        return 1;
    };
    if (!h_q || !h_radius || !h_scale) return fail("null argument");
    if (!(eps_in > 0.0) || !(eps_out > 0.0)) return fail("the solute and solvent dielectrics must be positive");
    if (!std::isfinite(sa_energy)) return fail("the surface-area energy is not finite");
    for (int i = 0; i < n; ++i) {
        if (!(h_radius[i] > AMM_GB_OFFSET) || !std::isfinite(h_radius[i]))
            return fail("particle " + std::to_string(i) + ": radius " + std::to_string(h_radius[i]) + " nm is not above the dielectric offset 0.009 nm");
        if (!(h_scale[i] >= 0.0) || !std::isfinite(h_scale[i])) return fail("particle " + std::to_string(i) + ": negative scale factor");
        if (!std::isfinite(h_q[i])) return fail("particle " + std::to_string(i) + ": charge is not finite");
    }
    return 0;
}

int amm_gb_set_params_impl(amm_ctx *ctx, GbForce *gb, const double *h_q, const double *h_radius, const double *h_scale, double eps_in,
                           double eps_out, double sa_energy, double rc) {
    const int n = gb->n;
    if (gb_check("amm_gb_set_params", n, h_q, h_radius, h_scale, eps_in, eps_out, sa_energy)) return 1;
    std::vector<double> rho(n), s(n), sa(n);
    const double four_pi = 4.0 * 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        const double R = h_radius[i];
        rho[i] = R - AMM_GB_OFFSET;
        s[i] = h_scale[i] * rho[i];
        const double R2 = R * R, p = R + AMM_GB_PROBE;
        sa[i] = four_pi * sa_energy * p * p * R2 * R2 * R2;
    }
    AMM_HIP(hipStreamSynchronize(ctx->stream));             // nothing in flight may still read the old values
    const size_t bytes = sizeof(double) * n;
    AMM_HIP(hipMemcpy(gb->d_q, h_q, bytes, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(gb->d_R, h_radius, bytes, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(gb->d_rho, rho.data(), bytes, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(gb->d_s, s.data(), bytes, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(gb->d_sa, sa.data(), bytes, hipMemcpyHostToDevice));
    gb->pre = 138.935456 * (1.0 / eps_in - 1.0 / eps_out);
    gb->rc2 = rc > 0.0 ? rc * rc : std::numeric_limits<double>::infinity();
    return 0;
}

int amm_gb_create_impl(amm_ctx *ctx, const double *h_q, const double *h_radius, const double *h_scale, double eps_in, double eps_out,
                       double sa_energy, double rc, GbForce **out) {
    const int n = ctx->n;
    if (n > AMM_FREE_MAX_ATOMS) {
        amm_set_error("amm_gb_create: a generalized-Born force walks all n^2 pairs three times and takes at most " +
                      std::to_string(AMM_FREE_MAX_ATOMS) + " atoms (this context has " + std::to_string(n) + ")");
        return 1;
    }
    if (ctx->world > 1) {
        amm_set_error("amm_gb_create: a generalized-Born force (AMM_FORCE_GB) runs on a single rank");
        return 1;
    }
    if (gb_check("amm_gb_create", n, h_q, h_radius, h_scale, eps_in, eps_out, sa_energy)) return 1;
    GbForce *gb = new GbForce();
    gb->n = n;
    const size_t bytes = sizeof(double) * n;
    double **arrays[] = {&gb->d_q, &gb->d_rho, &gb->d_s, &gb->d_R, &gb->d_sa, &gb->d_B, &gb->d_dBdI, &gb->d_g};
    bool ok = true;
    for (double **a : arrays) ok = ok && hipMalloc(a, bytes) == hipSuccess;
    ok = ok && hipMalloc(&gb->d_fdir, 3 * bytes) == hipSuccess;
    gb->n_epart = (n + 3) / 4;         // blocks at the widest rows (64 lanes: four rows per block): no allocation at evaluation time
    ok = ok && hipMalloc(&gb->d_epart, sizeof(double) * gb->n_epart) == hipSuccess;
    if (!ok) {
        amm_set_error("amm_gb_create: out of device memory");
        amm_gb_free(gb);
        return 1;
    }
    if (amm_gb_set_params_impl(ctx, gb, h_q, h_radius, h_scale, eps_in, eps_out, sa_energy, rc)) {
        amm_gb_free(gb);
        return 1;
    }
    *out = gb;
    return 0;
}

// lanes per row (the context's option, or free.hip's choice from n), as a shift; the blocks that cover n rows with it
static int gb_geometry(amm_ctx *ctx, int n, int &nblocks) {
    const int lpr = ctx->opt_gb_lpr > 0 ? ctx->opt_gb_lpr : amm_free_lanes_per_row(n);
    int shift = 0;
    while ((1 << shift) < lpr) ++shift;
    const int rows_per_block = AMM_GB_BLOCK >> shift;
    nblocks = (n + rows_per_block - 1) / rows_per_block;
    return shift;
}

static GbArgs gb_args(GbForce *gb, int shift, const double *d_pos, double *d_force, int accumulate) {
    GbArgs A;
    A.n = gb->n;
    A.lpr_shift = shift;
    A.wide = ((uintptr_t)d_pos & 15) == 0 ? 1 : 0;
    A.accumulate = accumulate;
    A.pos = d_pos;
    A.q = gb->d_q;
    A.rho = gb->d_rho;
    A.s = gb->d_s;
    A.R = gb->d_R;
    A.sa = gb->d_sa;
    A.B = gb->d_B;
    A.dBdI = gb->d_dBdI;
    A.g = gb->d_g;
    A.fdir = gb->d_fdir;
    A.force = d_force;
    A.epart = gb->d_epart;
    A.rc2 = gb->rc2;
    A.pre = gb->pre;
    return A;
}

int amm_gb_eval_impl(amm_ctx *ctx, GbForce *gb, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    hipStream_t st = ctx->stream;
    int nblocks = 0;
    const int shift = gb_geometry(ctx, gb->n, nblocks);
    const bool en = d_energy != nullptr;
    if (en && gb->n_epart < nblocks) {
        amm_set_error("generalized-Born force: more blocks than energy partials");      // (cannot happen: sized for 64 lanes per row)
        return 1;
    }
    const GbArgs A = gb_args(gb, shift, d_pos, d_force, accumulate);
    const dim3 grid(nblocks), block(AMM_GB_BLOCK);
    hipLaunchKernelGGL(k_gb_born, grid, block, 0, st, A);
    if (en) hipLaunchKernelGGL((k_gb_pair<true>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((k_gb_pair<false>), grid, block, 0, st, A);
    hipLaunchKernelGGL(k_gb_chain, grid, block, 0, st, A);
    AMM_HIP(hipGetLastError());
    gb->n_evals++;
    if (en) return amm_reduce_add(ctx, gb->d_epart, nblocks, 1.0, d_energy);
    return 0;
}

int amm_gb_born_radii_impl(amm_ctx *ctx, GbForce *gb, const double *d_pos, double *h_out) {
    int nblocks = 0;
    const int shift = gb_geometry(ctx, gb->n, nblocks);
    const GbArgs A = gb_args(gb, shift, d_pos, nullptr, 0);
    hipLaunchKernelGGL(k_gb_born, dim3(nblocks), dim3(AMM_GB_BLOCK), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    AMM_HIP(hipMemcpy(h_out, gb->d_B, sizeof(double) * gb->n, hipMemcpyDeviceToHost));
    return 0;
}

void amm_gb_free(GbForce *gb) {
    if (!gb) return;
    double *arrays[] = {gb->d_q, gb->d_rho, gb->d_s, gb->d_R, gb->d_sa, gb->d_B, gb->d_dBdI, gb->d_g, gb->d_fdir, gb->d_epart};
    for (double *a : arrays)
        if (a) (void)hipFree(a);
    delete gb;
}
