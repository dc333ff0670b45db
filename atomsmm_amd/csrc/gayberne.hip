// atomsmm_amd/csrc/gayberne.hip -- GayBerneForce (AMM_FORCE_GAYBERNE): the anisotropic pair potential of ellipsoids whose frames are
// defined by other particles (DESIGN.md 3.GY has the definition, the derivative chain and the measurements).
//
//   frame of i: x^ = d1 / |d1| with d1 = r_i - r_x; y^ = u / |u| with u = d2 - x^ (x^ . d2), d2 = r_i - r_y; z^ = x^ x y^ (minimum images
//   when periodic).  G_i = a^2 x^x^T + b^2 y^y^T + c^2 z^z^T with the radii a, b, c = sx/2, sy/2, sz/2; B_i the same with e_k^-1/2.
//   Without a y-particle (b = c, e_y = e_z) G_i = b^2 I + (a^2 - b^2) x^x^T needs no y^; without an x-particle both are multiples of I.
//   pair: G = G_i + G_j, B = B_i + B_j, kappa = G^-1 r^, q = r^ . kappa, sigma12 = sqrt(2 / q), iota = B^-1 r^, p = r^ . iota,
//   rho = sigma / (r - sigma12 + sigma), U = 4 eps (rho^12 - rho^6), eta = sqrt(2 s_i s_j / det G), chi = 4 p^2, E = U eta chi S(r).
//
// Four launches, every one owner-computes: no atomics, fp contraction off, all fp64, a fixed order of summation -- the same
// positions give the same bits.
//   k_gb_frames  one lane per ACTIVE particle (epsilon > 0, or in an exception with epsilon > 0; the caller compacts the list, so a
//                marker atom never enters the pair scan): the record of 18 doubles -- centre, the 6 + 6 unique entries of G_i and
//                B_i, s_i, sigma_i, sqrt(eps_i) -- and centre and sqrt(eps_i) once more, packed for the scan.
//   k_gb_pairs   one wavefront per active row i, or per chunk of its columns when the rows are few.  64 columns at a time are tested
//                against the cutoff and the row's exceptions (a CSR sorted by column, searched by bisection: any number per row);
//                the survivors queue up in LDS with ballot + prefix count and the heavy arithmetic -- two symmetric 3 x 3 inverses,
//                a determinant, the derivatives -- runs on full queues only, and once more at the row's end (the pattern of
//                hbond.hip).  A lane keeps the force on centre i, dE/dG_i, dE/dB_i and half the pair's energy; a fixed xor-shuffle
//                tree sums them and lane 0 parks 15 doubles per (row, chunk).  Every pair is evaluated from both sides.
//                The columns are not staged in LDS (a tile of 256 records is 36 KB for a block of one wavefront, which would leave
//                one wavefront per SIMD): the scan reads a packed copy of centre and sqrt(eps), 32 bytes a column and coalesced,
//                the arithmetic gathers the survivors' records from global memory.
//   k_gb_back    one lane per active row: the chunks in chunk order, then the chain rule through the frame -- dE/dx^, dE/dy^, dE/dz^
//                from dE/dG and dE/dB, z^ folded into x^ and y^, y^ into u, u into d2 AND x^ (the roll of the frame about x^ when
//                d2 is not perpendicular to d1), x^ into d1.  Parks the force on the centre (pairs and frame), on the x- and on the
//                y-particle.
//   k_gb_spread  one lane per particle of the context: its own centre record, then the x / y records of the ellipsoids that name it,
//                through a reverse CSR in index order.  Every force row is written exactly once.
// A degenerate frame (|d1| = 0, d2 parallel to d1) divides by zero: non-finite forces for the particles involved, nothing else.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "compound_geom.h"
#include "device_utils.h"
#include "expr_force.h"

#define AMM_GY_LANES 64
#define AMM_GY_MAX_ROWS 32768
#define AMM_GY_REC 18               // doubles of a record
#define AMM_GY_PARK 15              // doubles a (row, chunk) parks: force 3, dE/dG 6, dE/dB 6
#define AMM_GY_PAR 8                // per-particle parameters: sigma, epsilon, sx, sy, sz, ex, ey, ez

struct GayBerneForce {
    int n_act = 0, n_ex = 0, periodic = 0, cutoff = 0, use_switch = 0;
    double rc = 0.0, rs = 0.0;
    int chunks = 1, chunk_len = 64;
    int *d_active = nullptr;            // [n_act] particle of active row k, ascending
    int *d_axes = nullptr;              // [n_act][2] x- and y-particle, -1: none
    double *d_par = nullptr;            // [n_act][8]
    int *d_ex_ptr = nullptr, *d_ex_col = nullptr;   // CSR of a row's exceptions: columns (active indices), ascending
    double *d_ex_par = nullptr;         // [n_ex][2] sigma, epsilon of the CSR entry
    int *d_act_of = nullptr;            // [n] active row of a particle, -1: none
    int *d_rev_ptr = nullptr, *d_rev_src = nullptr; // CSR per particle of the (active row) * 2 + (0: x, 1: y) that name it
    double *d_rec = nullptr;            // [n_act][18]
    double4 *d_cen = nullptr;           // [n_act] centre and sqrt(eps) again, packed: what the scan reads of a column
    double *d_park = nullptr;           // [n_act * chunks][15]
    double *d_epart = nullptr;          // [n_act * chunks]
    int *d_count = nullptr;             // [n_act * chunks] surviving pairs of the last evaluation
    double *d_back = nullptr;           // [n_act][9] force on the centre, the x-particle, the y-particle
    std::vector<int> h_axes;            // the host's copy, for the checks of amm_gayberne_set_params
    long long launches = 0;
    bool evaluated = false;
};

struct GbArgs {
    int n, n_act, chunks, chunk_len, periodic, cutoff, use_switch, accumulate;
    double rc, rc2, rs;
    const int *active, *axes, *ex_ptr, *ex_col, *act_of, *rev_ptr, *rev_src;
    const double *par, *ex_par, *pos;
    double *rec, *park, *epart, *back, *force;
    double4 *cen;
    int *count;
    Box box;
};

// x^ (and with a y-particle y^, z^) of active row k; n1 = |d1|, nu = |u|, d2 as used
struct GbFrame {
    double x[3], y[3], z[3], d2[3], n1, nu;
};

__device__ __forceinline__ void gb_frame(const GbArgs &A, int i, int xp, int yp, GbFrame &F) {
#pragma clang fp contract(off)
    double d1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double v = A.pos[3 * (size_t)i + k] - A.pos[3 * (size_t)xp + k];
        if (A.periodic) v = amm_min_image(v, A.box.L[k], A.box.invL[k]);
        d1[k] = v;
    }
    F.n1 = sqrt(dot3(d1, d1));
#pragma unroll
    for (int k = 0; k < 3; ++k) F.x[k] = d1[k] / F.n1;
    if (yp < 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double v = A.pos[3 * (size_t)i + k] - A.pos[3 * (size_t)yp + k];
        if (A.periodic) v = amm_min_image(v, A.box.L[k], A.box.invL[k]);
        F.d2[k] = v;
    }
    const double xd = dot3(F.x, F.d2);
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = F.d2[k] - F.x[k] * xd;
    F.nu = sqrt(dot3(u, u));
#pragma unroll
    for (int k = 0; k < 3; ++k) F.y[k] = u[k] / F.nu;
    cross3(F.x, F.y, F.z);
}

// m (xx xy xz yy yz zz) += w v v^T
__device__ __forceinline__ void gb_add_outer(double *m, double w, const double *v) {
#pragma clang fp contract(off)
    m[0] += w * (v[0] * v[0]);
    m[1] += w * (v[0] * v[1]);
    m[2] += w * (v[0] * v[2]);
    m[3] += w * (v[1] * v[1]);
    m[4] += w * (v[1] * v[2]);
    m[5] += w * (v[2] * v[2]);
}

// out = M v for the symmetric M (xx xy xz yy yz zz)
__device__ __forceinline__ void gb_symv(const double *m, const double *v, double *out) {
#pragma clang fp contract(off)
    out[0] = (m[0] * v[0] + m[1] * v[1]) + m[2] * v[2];
    out[1] = (m[1] * v[0] + m[3] * v[1]) + m[4] * v[2];
    out[2] = (m[2] * v[0] + m[4] * v[1]) + m[5] * v[2];
}

__global__ void __launch_bounds__(256) k_gb_frames(GbArgs A) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_act) return;
    const int i = A.active[k], xp = A.axes[2 * k], yp = A.axes[2 * k + 1];
    const double *p = A.par + (size_t)AMM_GY_PAR * k;
    const double a = 0.5 * p[2], b = 0.5 * p[3], c = 0.5 * p[4];
    const double a2 = a * a, b2 = b * b, c2 = c * c;
    const double ea = 1.0 / sqrt(p[5]), eb = 1.0 / sqrt(p[6]), ec = 1.0 / sqrt(p[7]);
    double *r = A.rec + (size_t)AMM_GY_REC * k;
    double G[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, B[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (xp < 0) {
        G[0] = G[3] = G[5] = a2;
        B[0] = B[3] = B[5] = ea;
    } else {
        GbFrame F;
        gb_frame(A, i, xp, yp, F);
        if (yp < 0) {
            G[0] = G[3] = G[5] = b2;
            B[0] = B[3] = B[5] = eb;
            gb_add_outer(G, a2 - b2, F.x);
            gb_add_outer(B, ea - eb, F.x);
        } else {
            gb_add_outer(G, a2, F.x);
            gb_add_outer(G, b2, F.y);
            gb_add_outer(G, c2, F.z);
            gb_add_outer(B, ea, F.x);
            gb_add_outer(B, eb, F.y);
            gb_add_outer(B, ec, F.z);
        }
    }
    r[0] = A.pos[3 * (size_t)i];
    r[1] = A.pos[3 * (size_t)i + 1];
    r[2] = A.pos[3 * (size_t)i + 2];
#pragma unroll
    for (int x = 0; x < 6; ++x) {
        r[3 + x] = G[x];
        r[9 + x] = B[x];
    }
    r[15] = (a * b + c2) * sqrt(a * b);
    r[16] = p[0];
    r[17] = sqrt(p[1]);
    A.cen[k] = make_double4(r[0], r[1], r[2], r[17]);
}

// the inverse of the symmetric m (xx xy xz yy yz zz) by cofactors, and its determinant
__device__ __forceinline__ void gb_sym_inverse(const double *m, double *inv, double &det) {
#pragma clang fp contract(off)
    const double c0 = m[3] * m[5] - m[4] * m[4], c1 = m[2] * m[4] - m[1] * m[5], c2 = m[1] * m[4] - m[2] * m[3];
    const double c3 = m[0] * m[5] - m[2] * m[2], c4 = m[1] * m[2] - m[0] * m[4], c5 = m[0] * m[3] - m[1] * m[1];
    det = (m[0] * c0 + m[1] * c1) + m[2] * c2;
    const double w = 1.0 / det;
    inv[0] = c0 * w;
    inv[1] = c1 * w;
    inv[2] = c2 * w;
    inv[3] = c3 * w;
    inv[4] = c4 * w;
    inv[5] = c5 * w;
}

// index of x in list[lo, hi) (ascending), -1: not there
__device__ __forceinline__ int gb_sorted_find(const int *__restrict__ list, int lo, int hi, int x) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && list[lo] == x ? lo : -1;
}

__global__ void __launch_bounds__(AMM_GY_LANES) k_gb_pairs(GbArgs A) {
#pragma clang fp contract(off)
    __shared__ int2 s_queue[2 * AMM_GY_LANES];          // (column, exception entry or -1) of the pairs that wait for the arithmetic
    const int lane = threadIdx.x;
    const int row = blockIdx.x / A.chunks, chunk = blockIdx.x - row * A.chunks;     // (the grid is n_act * chunks)
    const int begin = min(chunk * A.chunk_len, A.n_act), end = min(begin + A.chunk_len, A.n_act);
    const double *ri = A.rec + (size_t)AMM_GY_REC * row;
    const double x0 = ri[0], y0 = ri[1], z0 = ri[2], s_i = ri[15], sig_i = ri[16], se_i = ri[17];
    const int ex_begin = A.ex_ptr[row], ex_end = A.ex_ptr[row + 1];
    double fc[3] = {0.0, 0.0, 0.0}, mg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double e_sum = 0.0;
    int n_pass = 0, qn = 0;
    for (int j0 = begin;; j0 += AMM_GY_LANES) {
        const bool last = j0 >= end;            // (wave-uniform: one more turn behind the columns, to drain what is left)
        if (!last) {
            const int col = j0 + lane;
            bool keep = col < end && col != row;
            int exi = -1;
            if (keep) {
                const double4 cj = A.cen[col];
                double dx = cj.x - x0, dy = cj.y - y0, dz = cj.z - z0;
                if (A.periodic) {
                    dx = amm_min_image(dx, A.box.L[0], A.box.invL[0]);
                    dy = amm_min_image(dy, A.box.L[1], A.box.invL[1]);
                    dz = amm_min_image(dz, A.box.L[2], A.box.invL[2]);
                }
                // (|r_j - r_i|^2 is the same number from either side: squares of negated differences)
                if (A.cutoff) keep = dx * dx + dy * dy + dz * dz < A.rc2;
                if (keep) {
                    if (ex_end > ex_begin) exi = gb_sorted_find(A.ex_col, ex_begin, ex_end, col);
                    keep = exi >= 0 ? A.ex_par[2 * (size_t)exi + 1] > 0.0 : se_i * cj.w > 0.0;     // epsilon 0: the pair is skipped
                }
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) s_queue[qn + __popcll(mask & ((1ull << lane) - 1ull))] = make_int2(col, exi);  // (qn < 64 here: at most 127 entries)
            qn += __popcll(mask);
            __syncthreads();
        }
        if (qn >= AMM_GY_LANES || (last && qn > 0)) {
            const int take = min(qn, AMM_GY_LANES);
            if (lane < take) {
                const int2 qe = s_queue[lane];
                const double *rj = A.rec + (size_t)AMM_GY_REC * qe.x;
                double d[3] = {rj[0] - x0, rj[1] - y0, rj[2] - z0};
                if (A.periodic) {
                    d[0] = amm_min_image(d[0], A.box.L[0], A.box.invL[0]);
                    d[1] = amm_min_image(d[1], A.box.L[1], A.box.invL[1]);
                    d[2] = amm_min_image(d[2], A.box.L[2], A.box.invL[2]);
                }
                const double r = sqrt(dot3(d, d));
                const double rh[3] = {d[0] / r, d[1] / r, d[2] / r};
                double sigma, eps;
                if (qe.y >= 0) {
                    sigma = A.ex_par[2 * (size_t)qe.y];
                    eps = A.ex_par[2 * (size_t)qe.y + 1];
                } else {
                    sigma = 0.5 * (sig_i + rj[16]);
                    eps = se_i * rj[17];
                }
                double m[6], inv[6], kap[3], iot[3], detG, detB;
#pragma unroll
                for (int x = 0; x < 6; ++x) m[x] = ri[3 + x] + rj[3 + x];
                gb_sym_inverse(m, inv, detG);
                gb_symv(inv, rh, kap);
                const double q = dot3(rh, kap);
                const double sig12 = sqrt(2.0 / q);
                const double rho = sigma / ((r - sig12) + sigma);
                const double rho2 = rho * rho, rho6 = rho2 * rho2 * rho2;
                const double U = 4.0 * eps * (rho6 * (rho6 - 1.0));
                const double dUdh = -(24.0 * eps / sigma) * ((rho6 * rho) * (2.0 * rho6 - 1.0));
                const double eta = sqrt(2.0 * (s_i * rj[15]) / detG);
                double S = 1.0, dS = 0.0;
                if (A.use_switch && r > A.rs) {
                    const double w = 1.0 / (A.rc - A.rs), t = (r - A.rs) * w;
                    S = 1.0 - (t * t * t) * (10.0 + t * (6.0 * t - 15.0));
                    dS = -30.0 * w * ((t * t) * ((1.0 - t) * (1.0 - t)));
                }
                const double ues = U * eta * S;                 // E = ues chi
                double mgi[6];                                  // G^-1 is kept; `m` and `inv` are taken again for B
#pragma unroll
                for (int x = 0; x < 6; ++x) mgi[x] = inv[x];
#pragma unroll
                for (int x = 0; x < 6; ++x) m[x] = ri[9 + x] + rj[9 + x];
                gb_sym_inverse(m, inv, detB);
                gb_symv(inv, rh, iot);
                const double p = dot3(rh, iot);
                const double chi = 4.0 * (p * p);
                const double E = ues * chi;
                const double dEdh = (eta * chi * S) * dUdh;
                const double dEdr = dEdh + (U * eta * chi) * dS;
                const double dEdq = dEdh * (0.25 * (sig12 * sig12 * sig12));
                const double dEdp = ues * (8.0 * p);
                const double wq = 2.0 * dEdq / r, wp = 2.0 * dEdp / r;
#pragma unroll
                for (int x = 0; x < 3; ++x) fc[x] += (dEdr * rh[x] + wq * (kap[x] - q * rh[x])) + wp * (iot[x] - p * rh[x]);
                gb_add_outer(mg, -dEdq, kap);
#pragma unroll
                for (int x = 0; x < 6; ++x) mg[x] += (-0.5 * E) * mgi[x];
                gb_add_outer(mb, -dEdp, iot);
                e_sum += 0.5 * E;
                ++n_pass;
            }
            qn = queue_keep_rest(s_queue, qn, take);        // what is left moves to the front
        }
        if (last) break;
    }
    for (int off = 32; off > 0; off >>= 1) {    // a fixed-order butterfly
#pragma unroll
        for (int x = 0; x < 3; ++x) fc[x] += __shfl_xor(fc[x], off);
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            mg[x] += __shfl_xor(mg[x], off);
            mb[x] += __shfl_xor(mb[x], off);
        }
        e_sum += __shfl_xor(e_sum, off);
        n_pass += __shfl_xor(n_pass, off);
    }
    if (lane == 0) {
        double *out = A.park + (size_t)blockIdx.x * AMM_GY_PARK;
#pragma unroll
        for (int x = 0; x < 3; ++x) out[x] = fc[x];
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            out[3 + x] = mg[x];
            out[9 + x] = mb[x];
        }
        A.epart[blockIdx.x] = e_sum;
        A.count[blockIdx.x] = n_pass;
    }
}

// one lane per active row: the chunks in chunk order, then dE/dG and dE/dB through the frame to d1 and d2
__global__ void __launch_bounds__(256) k_gb_back(GbArgs A) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_act) return;
    double s[AMM_GY_PARK];
    const double *pk = A.park + (size_t)k * A.chunks * AMM_GY_PARK;
#pragma unroll
    for (int x = 0; x < AMM_GY_PARK; ++x) s[x] = pk[x];
    for (int c = 1; c < A.chunks; ++c) {
#pragma unroll
        for (int x = 0; x < AMM_GY_PARK; ++x) s[x] += pk[(size_t)c * AMM_GY_PARK + x];
    }
    const int i = A.active[k], xp = A.axes[2 * k], yp = A.axes[2 * k + 1];
    double g1[3] = {0.0, 0.0, 0.0}, g2[3] = {0.0, 0.0, 0.0};       // dE/dd1, dE/dd2
    if (xp >= 0) {
        const double *p = A.par + (size_t)AMM_GY_PAR * k;
        const double a = 0.5 * p[2], b = 0.5 * p[3], c = 0.5 * p[4];
        const double a2 = a * a, b2 = b * b, c2 = c * c;
        const double ea = 1.0 / sqrt(p[5]), eb = 1.0 / sqrt(p[6]), ec = 1.0 / sqrt(p[7]);
        const double *MG = s + 3, *MB = s + 9;
        GbFrame F;
        gb_frame(A, i, xp, yp, F);
        double gx[3], tg[3], tb[3];
        gb_symv(MG, F.x, tg);
        gb_symv(MB, F.x, tb);
        if (yp < 0) {
#pragma unroll
            for (int x = 0; x < 3; ++x) gx[x] = 2.0 * ((a2 - b2) * tg[x] + (ea - eb) * tb[x]);
        } else {
            double gy[3], gz[3], t[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) gx[x] = 2.0 * (a2 * tg[x] + ea * tb[x]);
            gb_symv(MG, F.y, tg);
            gb_symv(MB, F.y, tb);
#pragma unroll
            for (int x = 0; x < 3; ++x) gy[x] = 2.0 * (b2 * tg[x] + eb * tb[x]);
            gb_symv(MG, F.z, tg);
            gb_symv(MB, F.z, tb);
#pragma unroll
            for (int x = 0; x < 3; ++x) gz[x] = 2.0 * (c2 * tg[x] + ec * tb[x]);
            // z^ = x^ x y^:  gz . (dx^ x y^) = dx^ . (y^ x gz),  gz . (x^ x dy^) = dy^ . (gz x x^)
            cross3(F.y, gz, t);
#pragma unroll
            for (int x = 0; x < 3; ++x) gx[x] += t[x];
            cross3(gz, F.x, t);
#pragma unroll
            for (int x = 0; x < 3; ++x) gy[x] += t[x];
            // y^ = u / |u|
            const double yg = dot3(F.y, gy);
            double gu[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) gu[x] = (gy[x] - F.y[x] * yg) / F.nu;
            // u = d2 - x^ (x^ . d2): on d2 directly, and on x^ -- the roll of the frame about x^
            const double gux = dot3(gu, F.x), xd = dot3(F.x, F.d2);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                g2[x] = gu[x] - F.x[x] * gux;
                gx[x] -= xd * gu[x] + gux * F.d2[x];
            }
        }
        // x^ = d1 / |d1|
        const double xg = dot3(F.x, gx);
#pragma unroll
        for (int x = 0; x < 3; ++x) g1[x] = (gx[x] - F.x[x] * xg) / F.n1;
    }
    double *out = A.back + (size_t)9 * k;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        out[x] = (s[x] - g1[x]) - g2[x];        // d1 = r_i - r_x, d2 = r_i - r_y
        out[3 + x] = g1[x];
        out[6 + x] = g2[x];
    }
}

// one lane per particle: its own centre, then the ellipsoids that name it as x- or y-particle, in index order
__global__ void __launch_bounds__(256) k_gb_spread(GbArgs A) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    const int k = A.act_of[i];
    if (k >= 0) {
        f0 = A.back[9 * (size_t)k];
        f1 = A.back[9 * (size_t)k + 1];
        f2 = A.back[9 * (size_t)k + 2];
    }
    const int re = A.rev_ptr[i + 1];
    for (int r = A.rev_ptr[i]; r < re; ++r) {
        const int src = A.rev_src[r];
        const double *p = A.back + 9 * (size_t)(src >> 1) + 3 + 3 * (src & 1);
        f0 += p[0];
        f1 += p[1];
        f2 += p[2];
    }
    store_force_row(A.force, i, f0, f1, f2, A.accumulate);
}

int amm_gayberne_eval_impl(amm_ctx *ctx, GayBerneForce *gf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    // (the box may have changed since creation: a barostat)
    if (gf->periodic && !amm_cutoff_fits_box(ctx, gf->rc, "Gay-Berne force (AMM_FORCE_GAYBERNE)")) return 1;
    GbArgs A;
    A.n = n;
    A.n_act = gf->n_act;
    A.chunks = gf->chunks;
    A.chunk_len = gf->chunk_len;
    A.periodic = gf->periodic;
    A.cutoff = gf->cutoff;
    A.use_switch = gf->use_switch;
    A.accumulate = accumulate ? 1 : 0;
    A.rc = gf->rc;
    A.rc2 = gf->rc * gf->rc;
    A.rs = gf->rs;
    A.active = gf->d_active;
    A.axes = gf->d_axes;
    A.ex_ptr = gf->d_ex_ptr;
    A.ex_col = gf->d_ex_col;
    A.act_of = gf->d_act_of;
    A.rev_ptr = gf->d_rev_ptr;
    A.rev_src = gf->d_rev_src;
    A.par = gf->d_par;
    A.ex_par = gf->d_ex_par;
    A.pos = d_pos;
    A.rec = gf->d_rec;
    A.cen = gf->d_cen;
    A.park = gf->d_park;
    A.epart = gf->d_epart;
    A.back = gf->d_back;
    A.force = d_force;
    A.count = gf->d_count;
    A.box = ctx->box;
    if (gf->n_act > 0) {
        const int per_row = (gf->n_act + 255) / 256;
        hipLaunchKernelGGL(k_gb_frames, dim3(per_row), dim3(256), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gb_pairs, dim3(gf->n_act * gf->chunks), dim3(AMM_GY_LANES), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gb_back, dim3(per_row), dim3(256), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
        gf->launches += 3;
        gf->evaluated = true;
    }
    // (a force without active particles still writes its rows: it may be the first member of its group)
    hipLaunchKernelGGL(k_gb_spread, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    gf->launches++;
    if (d_energy && gf->n_act > 0) return amm_reduce_add(ctx, gf->d_epart, gf->n_act * gf->chunks, 1.0, d_energy);
    return 0;
}

// ---- host ----
// the values of a parameter table and of the exceptions' table: what both amm_gayberne_create and amm_gayberne_set_params refuse
static int gb_check_values(const char *who, const int *axes, const double *h_par, int n_act, const double *h_ex_par, int n_ex) {
    auto fail = [who](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what + " (AMM_FORCE_GAYBERNE)");
        return 1;
    };
    for (int k = 0; k < n_act; ++k) {
        const double *p = h_par + (size_t)AMM_GY_PAR * k;
        const std::string row = " of active row " + std::to_string(k);
        for (int x = 0; x < AMM_GY_PAR; ++x)
            if (!std::isfinite(p[x])) return fail("parameter " + std::to_string(x) + row + " is not finite");
        if (p[0] < 0.0 || p[1] < 0.0) return fail("sigma or epsilon" + row + " is negative");
        for (int x = 2; x < AMM_GY_PAR; ++x)
            if (!(p[x] > 0.0)) return fail("a diameter or a well-depth scale" + row + " is not above zero");
        if (axes[2 * k] < 0 && !(p[2] == p[3] && p[3] == p[4] && p[5] == p[6] && p[6] == p[7]))
            return fail("no x-particle" + row + ", whose shape is not a sphere");
        if (axes[2 * k + 1] < 0 && !(p[3] == p[4] && p[6] == p[7])) return fail("no y-particle" + row + ", whose shape is not uniaxial");
    }
    for (int e = 0; e < n_ex; ++e) {
        const double sg = h_ex_par[2 * (size_t)e], ep = h_ex_par[2 * (size_t)e + 1];
        if (!std::isfinite(sg) || !std::isfinite(ep) || sg < 0.0 || ep < 0.0)
            return fail("sigma or epsilon of exception entry " + std::to_string(e) + " is negative or not finite");
    }
    return 0;
}

int amm_gayberne_create_impl(amm_ctx *ctx, const int32_t *h_active, int n_act, const int32_t *h_axes, const double *h_par, const int32_t *h_ex_ptr,
                             const int32_t *h_ex_col, const double *h_ex_par, const int32_t *h_rev_ptr, const int32_t *h_rev_src, double rc,
                             double rs, int periodic, GayBerneForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_gayberne_create: " + what + " (AMM_FORCE_GAYBERNE)");
        return 1;
    };
    const int n = ctx->n;
    if (ctx->world > 1) return fail("a Gay-Berne force runs on a single rank");
    if (n_act < 0) return fail("a negative count");
    if (n_act > AMM_GY_MAX_ROWS) return fail(std::to_string(n_act) + " interacting particles (limit " + std::to_string(AMM_GY_MAX_ROWS) + ")");
    if (!std::isfinite(rc) || !std::isfinite(rs) || rc < 0.0) return fail("the cutoff or the switching distance is not a distance");
    if (periodic && !(rc > 0.0)) return fail("CutoffPeriodic needs a cutoff distance above zero");
    if (periodic && !ctx->has_box) return fail("CutoffPeriodic, but the context has no periodic box");
    if (periodic && !amm_cutoff_fits_box(ctx, rc, "amm_gayberne_create")) return 1;
    if (rs >= 0.0 && !(rc > 0.0 && rs < rc)) return fail("the switching distance " + std::to_string(rs) + " lies outside [0, cutoff)");
    // the active list: ascending particles of the context; the axes: other particles of the context, or -1
    std::vector<int> act_of(n, -1);
    for (int k = 0; k < n_act; ++k) {
        const int i = h_active[k];
        if (i < 0 || i >= n) return fail("particle " + std::to_string(i) + " (active row " + std::to_string(k) + ") is out of range");
        if (k > 0 && i <= h_active[k - 1]) return fail("the active particles are not in ascending order at row " + std::to_string(k));
        act_of[i] = k;
        for (int r = 0; r < 2; ++r) {
            const int a = h_axes[2 * k + r];
            if (a < -1 || a >= n || a == i) return fail("axis particle " + std::to_string(a) + " of particle " + std::to_string(i) + " is out of range or the particle itself");
        }
        if (h_axes[2 * k] < 0 && h_axes[2 * k + 1] >= 0) return fail("particle " + std::to_string(i) + " has a y-particle and no x-particle");
    }
    // the exceptions: per row ascending columns, none the row itself, every pair on both rows with the same entry
    if (n_act > 0 && h_ex_ptr[0] != 0) return fail("the exceptions' row pointer does not start at 0");
    for (int k = 0; k < n_act; ++k)
        if (h_ex_ptr[k + 1] < h_ex_ptr[k]) return fail("the exceptions' row pointer decreases at row " + std::to_string(k));
    const int n_ex = n_act > 0 ? h_ex_ptr[n_act] : 0;
    auto find = [&](int row, int col) {
        const int32_t *b = h_ex_col + h_ex_ptr[row], *e = h_ex_col + h_ex_ptr[row + 1];
        const int32_t *it = std::lower_bound(b, e, col);
        return it != e && *it == col ? (int)(it - h_ex_col) : -1;
    };
    for (int k = 0; k < n_act; ++k)
        for (int e = h_ex_ptr[k]; e < h_ex_ptr[k + 1]; ++e) {
            const int c = h_ex_col[e];
            if (c < 0 || c >= n_act || c == k) return fail("exception column " + std::to_string(c) + " of row " + std::to_string(k) + " is out of range or the row itself");
            if (e > h_ex_ptr[k] && c <= h_ex_col[e - 1]) return fail("the exception columns of row " + std::to_string(k) + " are not ascending");
        }
    for (int k = 0; k < n_act; ++k)
        for (int e = h_ex_ptr[k]; e < h_ex_ptr[k + 1]; ++e) {
            const int m = find(h_ex_col[e], k);
            if (m < 0 || h_ex_par[2 * (size_t)m] != h_ex_par[2 * (size_t)e] || h_ex_par[2 * (size_t)m + 1] != h_ex_par[2 * (size_t)e + 1])
                return fail("the exception of rows " + std::to_string(k) + " and " + std::to_string(h_ex_col[e]) + " is not the same on both rows");
        }
    if (gb_check_values("amm_gayberne_create", h_axes, h_par, n_act, h_ex_par, n_ex)) return 1;
    // the reverse CSR: per particle the (row, role) that name it, ascending; every axis particle of an active row exactly once
    if (h_rev_ptr[0] != 0) return fail("the reverse table's row pointer does not start at 0");
    for (int i = 0; i < n; ++i)
        if (h_rev_ptr[i + 1] < h_rev_ptr[i]) return fail("the reverse table's row pointer decreases at particle " + std::to_string(i));
    int named = 0;
    for (int k = 0; k < 2 * n_act; ++k) named += h_axes[k] >= 0;
    if (h_rev_ptr[n] != named) return fail("the reverse table holds " + std::to_string(h_rev_ptr[n]) + " entries for " + std::to_string(named) + " axis particles");
    for (int i = 0; i < n; ++i)
        for (int r = h_rev_ptr[i]; r < h_rev_ptr[i + 1]; ++r) {
            const int src = h_rev_src[r];
            if (src < 0 || src >= 2 * n_act || h_axes[src] != i) return fail("reverse entry " + std::to_string(src) + " of particle " + std::to_string(i) + " does not name it");
            if (r > h_rev_ptr[i] && src <= h_rev_src[r - 1]) return fail("the reverse entries of particle " + std::to_string(i) + " are not ascending");
        }
    AMM_HIP(hipSetDevice(ctx->device));
    GayBerneForce *gf = new GayBerneForce();
    gf->n_act = n_act;
    gf->n_ex = n_ex;
    gf->periodic = periodic ? 1 : 0;
    gf->cutoff = rc > 0.0 ? 1 : 0;
    gf->use_switch = rs >= 0.0 ? 1 : 0;
    gf->rc = rc;
    gf->rs = rs >= 0.0 ? rs : 0.0;
    gf->h_axes.assign(h_axes, h_axes + 2 * (size_t)n_act);
    // a row is split into chunks of columns (a multiple of 64 each) when there are few rows: enough wavefronts to fill the device
    const int batches = std::max(1, (n_act + AMM_GY_LANES - 1) / AMM_GY_LANES);
    const int want = std::max(1, std::min((4096 + std::max(n_act, 1) - 1) / std::max(n_act, 1), batches));
    const int per = (batches + want - 1) / want;
    gf->chunk_len = per * AMM_GY_LANES;
    gf->chunks = (batches + per - 1) / per;
    auto alloc = [&]() {
        if (amm_upload(&gf->d_active, h_active, (size_t)n_act)) return 1;
        if (amm_upload(&gf->d_axes, h_axes, (size_t)n_act * 2)) return 1;
        if (amm_upload(&gf->d_par, h_par, (size_t)n_act * AMM_GY_PAR)) return 1;
        if (n_act > 0) {
            if (amm_upload(&gf->d_ex_ptr, h_ex_ptr, (size_t)n_act + 1)) return 1;
        } else {
            const int32_t zero = 0;
            if (amm_upload(&gf->d_ex_ptr, &zero, 1)) return 1;
        }
        if (amm_upload(&gf->d_ex_col, h_ex_col, (size_t)n_ex)) return 1;
        if (amm_upload(&gf->d_ex_par, h_ex_par, (size_t)n_ex * 2)) return 1;
        if (amm_upload(&gf->d_act_of, act_of.data(), act_of.size())) return 1;
        if (amm_upload(&gf->d_rev_ptr, h_rev_ptr, (size_t)n + 1)) return 1;
        if (amm_upload(&gf->d_rev_src, h_rev_src, (size_t)named)) return 1;
        const size_t rows = std::max<size_t>(n_act, 1), parts = rows * gf->chunks;
        AMM_HIP(hipMalloc(&gf->d_rec, sizeof(double) * rows * AMM_GY_REC));
        AMM_HIP(hipMalloc(&gf->d_cen, sizeof(double4) * rows));
        AMM_HIP(hipMalloc(&gf->d_park, sizeof(double) * parts * AMM_GY_PARK));
        AMM_HIP(hipMalloc(&gf->d_epart, sizeof(double) * parts));
        AMM_HIP(hipMalloc(&gf->d_count, sizeof(int) * parts));
        AMM_HIP(hipMalloc(&gf->d_back, sizeof(double) * rows * 9));
        AMM_HIP(hipMemset(gf->d_rec, 0, sizeof(double) * rows * AMM_GY_REC));
        AMM_HIP(hipMemset(gf->d_cen, 0, sizeof(double4) * rows));
        AMM_HIP(hipMemset(gf->d_park, 0, sizeof(double) * parts * AMM_GY_PARK));
        AMM_HIP(hipMemset(gf->d_epart, 0, sizeof(double) * parts));
        AMM_HIP(hipMemset(gf->d_count, 0, sizeof(int) * parts));
        AMM_HIP(hipMemset(gf->d_back, 0, sizeof(double) * rows * 9));
        return 0;
    };
    if (alloc()) {
        amm_gayberne_free(gf);
        return 1;
    }
    *out = gf;
    return 0;
}

// a refused call leaves the force as it was: the checks come before anything is copied
int amm_gayberne_set_params_impl(amm_ctx *ctx, GayBerneForce *gf, const double *h_par, int n_act, const double *h_ex_par, int n_ex) {
    if (n_act != gf->n_act || n_ex != gf->n_ex || (n_act > 0 && !h_par) || (n_ex > 0 && !h_ex_par)) {
        amm_set_error("amm_gayberne_set_params: the force has " + std::to_string(gf->n_act) + " active particles and " + std::to_string(gf->n_ex) +
                      " exception entries, " + std::to_string(n_act) + " and " + std::to_string(n_ex) + " given (AMM_FORCE_GAYBERNE)");
        return 1;
    }
    if (gb_check_values("amm_gayberne_set_params", gf->h_axes.data(), h_par, n_act, h_ex_par, n_ex)) return 1;
    AMM_HIP(hipSetDevice(ctx->device));
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (n_act) AMM_HIP(hipMemcpy(gf->d_par, h_par, sizeof(double) * AMM_GY_PAR * (size_t)n_act, hipMemcpyHostToDevice));
    if (n_ex) AMM_HIP(hipMemcpy(gf->d_ex_par, h_ex_par, sizeof(double) * 2 * (size_t)n_ex, hipMemcpyHostToDevice));
    return 0;
}

// out[0]: active rows; out[1]: ordered pairs the scan tests (each pair from both sides); out[2]: those that passed the cutoff and the
// exceptions in the last evaluation; out[3]: launches so far; out[4]: chunks per row
int amm_gayberne_stats_impl(amm_ctx *ctx, GayBerneForce *gf, int64_t out[5]) {
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t parts = (size_t)gf->n_act * gf->chunks;
    long long kept = 0;
    if (gf->evaluated && parts) {
        std::vector<int> count(parts);
        AMM_HIP(hipMemcpy(count.data(), gf->d_count, sizeof(int) * parts, hipMemcpyDeviceToHost));
        for (int c : count) kept += c;
    }
    out[0] = gf->n_act;
    out[1] = (int64_t)gf->n_act * std::max(gf->n_act - 1, 0);
    out[2] = kept;
    out[3] = gf->launches;
    out[4] = gf->chunks;
    return 0;
}

void amm_gayberne_free(GayBerneForce *gf) {
    if (!gf) return;
    for (void *p : {(void *)gf->d_active, (void *)gf->d_axes, (void *)gf->d_par, (void *)gf->d_ex_ptr, (void *)gf->d_ex_col, (void *)gf->d_ex_par,
                    (void *)gf->d_act_of, (void *)gf->d_rev_ptr, (void *)gf->d_rev_src, (void *)gf->d_rec, (void *)gf->d_cen, (void *)gf->d_park, (void *)gf->d_epart,
                    (void *)gf->d_count, (void *)gf->d_back})
        if (p) (void)hipFree(p);
    delete gf;
}
