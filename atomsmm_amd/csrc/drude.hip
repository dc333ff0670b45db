// atomsmm_amd/csrc/drude.hip -- Drude oscillators: the force of a DrudeForce (AMM_FORCE_DRUDE) and the dual-thermostat step of a
// DrudeLangevinIntegrator (AMM_OP_DRUDE_STEP) (gfx950, fp64).
//
// The formulas are those of OpenMM's Reference platform, restated [recalled -- OpenMM's sources are not at hand; as in stock.hip and
// constraints.hip].  K = 138.935456, the Coulomb constant of every Coulomb term of this library.
//
// FORCE.  A Drude particle (p, p1, p2, p3, p4, q, alpha, a12, a34): a1 = a12 if p2 != -1 else 1; a2 = a34 if p3, p4 != -1 else 1;
// a3 = 3 - a1 - a2; k3 = K q^2/(alpha a3), k1 = K q^2/(alpha a1) - k3, k2 = K q^2/(alpha a2) - k3; with d = x_p - x_p1
//   E = 1/2 k3 |d|^2 + [p2] 1/2 k1 (d.u1)^2 + [p3, p4] 1/2 k2 (d.u2)^2,  u1 = unit(x_p1 - x_p2), u2 = unit(x_p3 - x_p4)
// and the forces are the exact gradient, the rotation of u1, u2 included: with s = d.u and L the length behind u,
//   dE/dd = k s u  (on p, minus it on p1)   and   dE/db = k s (d - s u)/L  (on the head of b, minus it on its tail).
// A screened pair (Drude entries A, B, thole t): s = t/(alpha_A alpha_B)^(1/6); the sites of an entry are its Drude particle with
// charge q and its parent with charge -q; for the four site pairs (i, j), r = |x_i - x_j|, u = s r, S(u) = 1 - (1 + u/2) exp(-u):
//   E += K q_i q_j S/r ,  dE/dr = K q_i q_j (s (1 + u)/2 exp(-u)/r - S/r^2).
// Displacements are raw, or each its own minimum image in the orthorhombic box (periodic).
//
// Two launches, no atomics, the pattern of cmap.hip: k_drude evaluates one spring or one screened pair per lane (the two classes start
// at multiples of the wavefront size, so a wavefront never holds both) and parks the forces of its roles -- five for a spring, four
// for a pair; k_drude_gather, one lane per atom, adds the atom's parked slots in slot order from a CSR built at creation and writes
// every row when it does not accumulate.  The energy: a fixed-order reduction per block into partials, which the first wavefront of
// the gather launch adds in a fixed order.  fp contraction is off: the same positions give the same bits.
// A force has as many springs as the System has polarizable atoms -- one per water -- so at 4 096 waters the launch is 16 blocks:
// bound by the launch and the latency of two dependent reads (atoms, positions), not by fp64 throughput.
//
// STEP.  With a = exp(-gamma dt), b = (1 - a)/gamma (dt when gamma = 0), a_D, b_D likewise from gamma_D, f the forces at x, N =
// amm_gaussian(seed, counter, dof) with one counter per op (the stream of AMM_OP_STOCK):
//   ordinary massive atom   v1 = a v + b f/m + sqrt(kT (1 - a^2)/m) N          -- the arithmetic of AMM_STOCK_LANGEVIN, operation by operation
//   pair (Drude p of mass m1, parent p1 of mass m2, M = m1 + m2, mu = m1 m2/M)
//       v_cm = (m1 v_p + m2 v_p1)/M, v_rel = v_p - v_p1, f_cm = f_p + f_p1, f_rel = f_p m2/M - f_p1 m1/M
//       v_cm  <- a v_cm + b f_cm/M + sqrt(kT (1 - a^2)/M) N[3 p1 + j]
//       v_rel <- a_D v_rel + b_D f_rel/mu + sqrt(kT_D (1 - a_D^2)/mu) N[3 p + j]
//       v_p = v_cm + v_rel m2/M, v_p1 = v_cm - v_rel m1/M
//   x' = x + dt v1 ; SHAKE x' along the bond vectors of x ; v = (x' - x)/dt ; massless particles never move
//   hard wall (R > 0), per pair: d = x_p - x_p1, r = |d|, n = d/r, delta = r - R; r <= R: nothing; r > 2 R: the pair is flagged
//   (amm_check fails); else the velocities along n (w_p, w_p1) lose their mass-weighted mean wbar, tau = min(dt, delta/|w_p - w_p1|)
//   (dt if equal), c = sqrt(kT_D/m1), w_p <- -sign(w_p) c m2/M, w_p1 <- -sign(w_p1) c m1/M, x_p += n (-delta m2/M + tau w_p),
//   x_p1 += n (delta m1/M + tau w_p1), wbar is added back.  A massless parent: w_p <- -sign(w_p) c, x_p += n (-delta + tau w_p),
//   tau = min(dt, delta/|w_p|).  A Drude particle whose parent is massless, or a massless Drude particle's parent, is thermalised as
//   an ordinary atom.
// ONE launch, the mapping of stock.hip: the work unit is a constraint cluster (or an atom of no cluster) TOGETHER WITH the Drude
// particles whose parents it holds, and one thread carries it from the loads to the stores.  A Drude particle is never constrained,
// so as a unit of its own it returns at once: its parent's unit moves it.  The rigid triangle with up to one Drude particle per
// vertex (the water shape) and the lone pair (an atom of no cluster with its Drude particle) are instantiations whose array indices
// are compile-time constants: registers only.  Other clusters take the generic sweep in the same launch (arrays in scratch memory);
// a constraint set without them launches the instantiation without that path.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "amm_ctx.h"
#include "cons_sweeps.h"
#include "bonded_terms.h"
#include "device_utils.h"
#include "expr_vm.h"

#define AMM_DRUDE_BLOCK 256
static constexpr double kDrudeKc = 138.935456;

struct DrudeForce {
    int n_spring = 0, n_pair = 0, periodic = 0, n_blocks = 1, o_pair = 0, total = 0;
    std::vector<int> h_idx;            // [n_spring][5], kept to check set_params against
    int *d_idx = nullptr;              // [n_spring][5] p, p1, p2, p3, p4 (-1: none)
    double *d_k = nullptr;             // [n_spring][3] k1, k2, k3
    int *d_pidx = nullptr;             // [n_pair][4] the sites: Drude and parent of entry A, of entry B
    std::vector<int> h_pent;           // [n_pair][2] the Drude entries of a pair
    double *d_ppar = nullptr;          // [n_pair][3] K q_A q_B, s, 0
    double *d_park = nullptr;          // [n_spring][5][3] then [n_pair][4][3] parked forces
    double *d_epart = nullptr;         // [n_blocks]
    int *d_ref_ptr = nullptr;          // [n + 1]: CSR of the parked slots of an atom ...
    int *d_rec_src = nullptr;          // ... ascending
};

struct DrudeArgs {
    int n_spring, n_pair, o_pair, periodic;
    const int *idx;
    const double *k;
    const int *pidx;
    const double *ppar;
    const double *pos;
    double *park;
    double *epart;
    Box box;
};

// 1/2 k (d.u)^2 with u = unit(b): adds dE/dd to gd and leaves dE/db in gb; returns the energy
__device__ __forceinline__ double drude_aniso(double k, const double *d, const double *b, double *gd, double *gb) {
#pragma clang fp contract(off)
    const double L = sqrt(dot3(b, b));
    double u[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) u[x] = b[x] / L;
    const double s = dot3(d, u);
    const double ks = k * s;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        gd[x] += ks * u[x];
        gb[x] = ks * (d[x] - s * u[x]) / L;
    }
    return 0.5 * k * s * s;
}

template <bool EN>
__global__ void __launch_bounds__(AMM_DRUDE_BLOCK) k_drude(DrudeArgs A) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const PosPlain pos{A.pos};
    double e = 0.0;
    if (t < A.n_spring) {
        int ix[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) ix[r] = A.idx[5 * (size_t)t + r];
        const double k1 = A.k[3 * (size_t)t], k2 = A.k[3 * (size_t)t + 1], k3 = A.k[3 * (size_t)t + 2];
        double d[3], gd[3], g2[3] = {0.0, 0.0, 0.0}, g34[3] = {0.0, 0.0, 0.0};
        delta3(pos, ix[0], ix[1], A.box, A.periodic, d);
        e = 0.5 * k3 * dot3(d, d);
#pragma unroll
        for (int x = 0; x < 3; ++x) gd[x] = k3 * d[x];
        if (ix[2] >= 0) {
            double b[3];
            delta3(pos, ix[1], ix[2], A.box, A.periodic, b);
            e += drude_aniso(k1, d, b, gd, g2);
        }
        if (ix[3] >= 0 && ix[4] >= 0) {
            double b[3];
            delta3(pos, ix[3], ix[4], A.box, A.periodic, b);
            e += drude_aniso(k2, d, b, gd, g34);
        }
        // gd = dE/dd (d = x_p - x_p1), g2 = dE/db1 (b1 = x_p1 - x_p2), g34 = dE/db2 (b2 = x_p3 - x_p4)
        double *out = A.park + (size_t)t * 15;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            out[x] = -gd[x];
            out[3 + x] = gd[x] - g2[x];
            out[6 + x] = g2[x];
            out[9 + x] = -g34[x];
            out[12 + x] = g34[x];
        }
    } else if (t >= A.o_pair && t - A.o_pair < A.n_pair) {
        const int q = t - A.o_pair;
        int ix[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ix[r] = A.pidx[4 * (size_t)q + r];
        const double kqq = A.ppar[3 * (size_t)q], s = A.ppar[3 * (size_t)q + 1];
        double fo[4][3] = {};
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const double qq = (a == b) ? kqq : -kqq;         // Drude q, parent -q
                double dv[3];
                delta3(pos, ix[a], ix[2 + b], A.box, A.periodic, dv);
                const double r2 = dot3(dv, dv), r = sqrt(r2);
                const double u = s * r, ex = exp(-u);
                const double S = 1.0 - (1.0 + 0.5 * u) * ex;
                e += qq * S / r;
                const double dEdr = qq * (s * (0.5 * (1.0 + u)) * ex / r - S / r2);
                const double c = dEdr / r;
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const double g = c * dv[x];
                    fo[a][x] -= g;
                    fo[2 + b][x] += g;
                }
            }
        }
        double *out = A.park + (size_t)A.n_spring * 15 + (size_t)q * 12;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int x = 0; x < 3; ++x) out[3 * r + x] = fo[r][x];
    }
    if (EN) block_energy_store_256(e, A.epart);
}

// one lane per atom: its parked slots, in slot order; the first wavefront of the launch adds the energy partials in a fixed order
template <bool EN>
__global__ void __launch_bounds__(256) k_drude_gather(int n, const int *__restrict__ ref_ptr, const int *__restrict__ rec_src,
                                                      const double *__restrict__ park, double *__restrict__ force, int accumulate,
                                                      const double *__restrict__ epart, int n_part, double *energy) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (EN && blockIdx.x == 0 && threadIdx.x < 64) {
        double e = 0.0;
        for (int b = threadIdx.x; b < n_part; b += 64) e += epart[b];
        for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
        if (threadIdx.x == 0) *energy += e;
    }
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

int amm_drude_eval_impl(amm_ctx *ctx, DrudeForce *df, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    const bool terms = df->total > 0;
    if (terms) {
        DrudeArgs A;
        A.n_spring = df->n_spring;
        A.n_pair = df->n_pair;
        A.o_pair = df->o_pair;
        A.periodic = df->periodic;
        A.idx = df->d_idx;
        A.k = df->d_k;
        A.pidx = df->d_pidx;
        A.ppar = df->d_ppar;
        A.pos = d_pos;
        A.park = df->d_park;
        A.epart = df->d_epart;
        A.box = ctx->box;
        if (d_energy) hipLaunchKernelGGL((k_drude<true>), dim3(df->n_blocks), dim3(AMM_DRUDE_BLOCK), 0, ctx->stream, A);
        else hipLaunchKernelGGL((k_drude<false>), dim3(df->n_blocks), dim3(AMM_DRUDE_BLOCK), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
    }
    // (a force without terms still writes its rows: it may be the first member of its group)
    const dim3 grid(std::max(1, (n + 255) / 256));
    if (d_energy && terms)
        hipLaunchKernelGGL((k_drude_gather<true>), grid, dim3(256), 0, ctx->stream, n, df->d_ref_ptr, df->d_rec_src, df->d_park, d_force, accumulate,
                           df->d_epart, df->n_blocks, d_energy);
    else
        hipLaunchKernelGGL((k_drude_gather<false>), grid, dim3(256), 0, ctx->stream, n, df->d_ref_ptr, df->d_rec_src, df->d_park, d_force,
                           accumulate, df->d_epart, 0, d_energy);
    AMM_HIP(hipGetLastError());
    return 0;
}

// ---- host ----
// the spring constants and the pair parameters from the rows of the object model; 1: refused (the message is set)
static int drude_params(const char *who, int n_spring, const int32_t *h_idx, const double *h_par, int n_pair, const int32_t *h_pent,
                        const double *h_thole, std::vector<double> &k, std::vector<double> &ppar) {
    auto fail = [&](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what + " (AMM_FORCE_DRUDE)");
        return 1;
    };
    k.assign((size_t)n_spring * 3, 0.0);
    ppar.assign((size_t)n_pair * 3, 0.0);
    for (int t = 0; t < n_spring; ++t) {
        const int32_t *ix = h_idx + 5 * (size_t)t;
        const double q = h_par[4 * (size_t)t], alpha = h_par[4 * (size_t)t + 1];
        const double a1 = ix[2] != -1 ? h_par[4 * (size_t)t + 2] : 1.0;
        const double a2 = (ix[3] != -1 && ix[4] != -1) ? h_par[4 * (size_t)t + 3] : 1.0;
        const double a3 = 3.0 - a1 - a2;
        if (!(alpha > 0.0)) return fail("Drude particle " + std::to_string(t) + " needs a polarizability above zero");
        if (!(a1 > 0.0) || !(a2 > 0.0) || !(a3 > 0.0)) return fail("Drude particle " + std::to_string(t) + " needs aniso12, aniso34 and 3 - aniso12 - aniso34 above zero");
        const double kq = kDrudeKc * q * q;
        const double k3 = kq / (alpha * a3);
        k[3 * (size_t)t] = kq / (alpha * a1) - k3;
        k[3 * (size_t)t + 1] = kq / (alpha * a2) - k3;
        k[3 * (size_t)t + 2] = k3;
    }
    for (int p = 0; p < n_pair; ++p) {
        const int a = h_pent[2 * (size_t)p], b = h_pent[2 * (size_t)p + 1];
        if (a < 0 || a >= n_spring || b < 0 || b >= n_spring || a == b)
            return fail("screened pair " + std::to_string(p) + " names a Drude particle that does not exist, or one twice");
        const double qa = h_par[4 * (size_t)a], qb = h_par[4 * (size_t)b], aa = h_par[4 * (size_t)a + 1], ab = h_par[4 * (size_t)b + 1];
        ppar[3 * (size_t)p] = kDrudeKc * qa * qb;
        ppar[3 * (size_t)p + 1] = h_thole[p] / pow(aa * ab, 1.0 / 6.0);
    }
    return 0;
}

int amm_drude_create_impl(amm_ctx *ctx, const int32_t *h_idx, const double *h_par, int n_spring, const int32_t *h_pent, const double *h_thole,
                          int n_pair, int periodic, DrudeForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_drude_create: " + what + " (AMM_FORCE_DRUDE)");
        return 1;
    };
    const int n = ctx->n;
    if (n_spring < 0 || n_pair < 0) return fail("a negative count");
    if (periodic && !ctx->has_box) return fail("periodic displacements, but the context has no periodic box");
    if (ctx->world > 1) return fail("a Drude force runs on a single rank");
    if ((long long)n_spring * 5 + (long long)n_pair * 4 > (long long)INT_MAX / 4) return fail("too many parked slots for a 32-bit index");
    for (int t = 0; t < n_spring; ++t) {
        const int32_t *ix = h_idx + 5 * (size_t)t;
        if (ix[0] < 0 || ix[0] >= n || ix[1] < 0 || ix[1] >= n || ix[0] == ix[1])
            return fail("Drude particle " + std::to_string(t) + ": the particle or its parent is out of range, or they are the same");
        for (int r = 2; r < 5; ++r)
            if (ix[r] < -1 || ix[r] >= n) return fail("Drude particle " + std::to_string(t) + ": an anisotropy particle is out of range");
        if (ix[2] == ix[1] || (ix[3] >= 0 && ix[3] == ix[4]))
            return fail("Drude particle " + std::to_string(t) + ": an anisotropy direction joins a particle to itself");
    }
    std::vector<double> k, ppar;
    if (drude_params("amm_drude_create", n_spring, h_idx, h_par, n_pair, h_pent, h_thole, k, ppar)) return 1;
    AMM_HIP(hipSetDevice(ctx->device));
    DrudeForce *df = new DrudeForce();
    df->n_spring = n_spring;
    df->n_pair = n_pair;
    df->periodic = periodic ? 1 : 0;
    df->o_pair = (n_spring + 63) / 64 * 64;
    df->total = n_pair > 0 ? df->o_pair + n_pair : n_spring;
    df->n_blocks = std::max(1, (df->total + AMM_DRUDE_BLOCK - 1) / AMM_DRUDE_BLOCK);
    df->h_idx.assign(h_idx, h_idx + (size_t)n_spring * 5);
    df->h_pent.assign(h_pent, h_pent + (size_t)n_pair * 2);
    std::vector<int> pidx((size_t)n_pair * 4);
    for (int p = 0; p < n_pair; ++p)
        for (int e = 0; e < 2; ++e) {
            const int32_t *ix = h_idx + 5 * (size_t)h_pent[2 * (size_t)p + e];
            pidx[4 * (size_t)p + 2 * e] = ix[0];
            pidx[4 * (size_t)p + 2 * e + 1] = ix[1];
        }
    // CSR of the parked slots per atom, ascending: the springs' (a role whose particle is -1 has no slot), then the pairs'
    const size_t n_slot = (size_t)n_spring * 5 + (size_t)n_pair * 4;
    std::vector<int> atom_of(n_slot);
    for (size_t s = 0; s < (size_t)n_spring * 5; ++s) {
        const int r = (int)(s % 5);
        int a = h_idx[s];
        if (r >= 3 && (h_idx[s - r + 3] < 0 || h_idx[s - r + 4] < 0)) a = -1;      // (p3 without p4: the direction is not used)
        atom_of[s] = a;
    }
    for (size_t s = 0; s < (size_t)n_pair * 4; ++s) atom_of[(size_t)n_spring * 5 + s] = pidx[s];
    std::vector<int> ptr(n + 1, 0), src;
    for (size_t s = 0; s < n_slot; ++s)
        if (atom_of[s] >= 0) ptr[atom_of[s] + 1]++;
    for (int i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    src.resize(ptr[n]);
    {
        std::vector<int> fill(ptr.begin(), ptr.end() - 1);
        for (size_t s = 0; s < n_slot; ++s)
            if (atom_of[s] >= 0) src[fill[atom_of[s]]++] = (int)s;
    }
    auto alloc = [&]() {
        if (amm_upload(&df->d_idx, df->h_idx.data(), df->h_idx.size())) return 1;
        if (amm_upload(&df->d_k, k.data(), k.size())) return 1;
        if (amm_upload(&df->d_pidx, pidx.data(), pidx.size())) return 1;
        if (amm_upload(&df->d_ppar, ppar.data(), ppar.size())) return 1;
        if (amm_upload(&df->d_ref_ptr, ptr.data(), ptr.size())) return 1;
        if (amm_upload(&df->d_rec_src, src.data(), src.size())) return 1;
        const size_t park = std::max<size_t>(n_slot * 3, 1);
        AMM_HIP(hipMalloc(&df->d_park, sizeof(double) * park));
        AMM_HIP(hipMemset(df->d_park, 0, sizeof(double) * park));
        AMM_HIP(hipMalloc(&df->d_epart, sizeof(double) * df->n_blocks));
        AMM_HIP(hipMemset(df->d_epart, 0, sizeof(double) * df->n_blocks));
        return 0;
    };
    if (alloc()) {
        amm_drude_free(df);
        return 1;
    }
    *out = df;
    return 0;
}

int amm_drude_set_params_impl(amm_ctx *ctx, DrudeForce *df, const int32_t *h_idx, const double *h_par, int n_spring, const int32_t *h_pent,
                              const double *h_thole, int n_pair) {
    if (n_spring != df->n_spring || n_pair != df->n_pair) {
        amm_set_error("amm_drude_set_params: the force has " + std::to_string(df->n_spring) + " Drude particles and " + std::to_string(df->n_pair) +
                      " screened pairs, " + std::to_string(n_spring) + " and " + std::to_string(n_pair) + " given (AMM_FORCE_DRUDE)");
        return 1;
    }
    if ((n_spring > 0 && (!h_idx || !h_par)) || (n_pair > 0 && (!h_pent || !h_thole))) {
        amm_set_error("amm_drude_set_params: null argument");
        return 1;
    }
    if ((n_spring && memcmp(h_idx, df->h_idx.data(), sizeof(int) * df->h_idx.size()) != 0) ||
        (n_pair && memcmp(h_pent, df->h_pent.data(), sizeof(int) * df->h_pent.size()) != 0)) {
        amm_set_error("amm_drude_set_params: the particles of a Drude particle or of a screened pair have changed; only values may (AMM_FORCE_DRUDE)");
        return 1;
    }
    std::vector<double> k, ppar;
    if (drude_params("amm_drude_set_params", n_spring, h_idx, h_par, n_pair, h_pent, h_thole, k, ppar)) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));     // ordered after any kernel already queued on the stream that reads the old values
    if (n_spring) AMM_HIP(hipMemcpy(df->d_k, k.data(), sizeof(double) * k.size(), hipMemcpyHostToDevice));
    if (n_pair) AMM_HIP(hipMemcpy(df->d_ppar, ppar.data(), sizeof(double) * ppar.size(), hipMemcpyHostToDevice));
    return 0;
}

void amm_drude_free(DrudeForce *df) {
    if (!df) return;
    for (void *p : {(void *)df->d_idx, (void *)df->d_k, (void *)df->d_pidx, (void *)df->d_ppar, (void *)df->d_park, (void *)df->d_epart,
                    (void *)df->d_ref_ptr, (void *)df->d_rec_src})
        if (p) (void)hipFree(p);
    delete df;
}

// ================================================================ the step ================================================================
struct DrudeStepArgs {
    int n_tri, n_two, n_gen, n_free;
    int o_two, o_gen, o_free, total;
    const int *units, *fixed, *cptr, *aptr, *atoms;
    const int2 *pair;
    const double *dist;
    double tol;
    int *fail;
    double *x, *v, *xref;
    const double *f, *mass;
    const int *drude_of, *parent_of;       // per atom: the Drude particle it is the parent of / the parent it is the Drude particle of (-1: none)
    int *flag;                             // set when a pair is beyond twice the hard wall
    DrudeStepDef D;
    unsigned long long seed, counter;
    WatchArgs W;
};

// one unit: atoms idx[0 .. na) and the Drude particle of each (dk[k], -1: none)
template <class S>
__device__ __forceinline__ void drude_unit(const DrudeStepArgs &A, const S &s, const int (&idx)[S::NA], int na) {
#pragma clang fp contract(off)
    constexpr int NA = S::NA;
    const DrudeStepDef &D = A.D;
    const double dt = D.dt;
    double x0[NA][3], p[NA][3], w[NA][3], im[NA], ms[NA];
    double xd0[NA][3], pd[NA][3], wd[NA][3], md[NA];
    int dk[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
            const int i = idx[k];
            const double m = A.mass[i];
            ms[k] = m;
            im[k] = 1.0 / m;
            const int dr = A.drude_of[i];
            dk[k] = dr;
            const double m1 = dr >= 0 ? A.mass[dr] : 0.0;
            md[k] = m1;
            const bool both = dr >= 0 && m1 > 0.0 && m > 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = 3 * i + j;
                const double xt = A.x[t], vt = A.v[t], ft = A.f[t];
                x0[k][j] = xt;
                p[k][j] = xt;
                w[k][j] = vt;
                if (dr >= 0) {
                    const int td = 3 * dr + j;
                    const double xq = A.x[td], vq = A.v[td], fq = A.f[td];
                    xd0[k][j] = xq;
                    pd[k][j] = xq;
                    wd[k][j] = vq;
                    if (both) {
                        const double M = m1 + m, mu = m1 * m / M;
                        const double r2 = m / M, r1 = m1 / M;
                        const double vcm = (m1 * vq + m * vt) / M, vrel = vq - vt;
                        const double fcm = fq + ft, frel = fq * r2 - ft * r1;
                        const double gc = amm_gaussian(A.seed, A.counter, (unsigned)t);
                        const double gr = amm_gaussian(A.seed, A.counter, (unsigned)td);
                        const double ncm = (D.a * vcm + D.b * fcm / M) + sqrt(D.kT * (1.0 - D.a * D.a) / M) * gc;
                        const double nrel = (D.aD * vrel + D.bD * frel / mu) + sqrt(D.kTD * (1.0 - D.aD * D.aD) / mu) * gr;
                        wd[k][j] = ncm + nrel * r2;
                        w[k][j] = ncm - nrel * r1;
                    } else if (m1 > 0.0) {          // (a massless parent: the Drude particle is an ordinary atom)
                        const double g = amm_gaussian(A.seed, A.counter, (unsigned)td);
                        const double av = D.a * vq;
                        const double bf = D.b * fq;
                        const double drift = av + bf / m1;
                        const double var = D.kT * (1.0 - D.a * D.a);
                        const double amp = sqrt(var / m1);
                        wd[k][j] = drift + amp * g;
                    }
                }
                if (!both && m > 0.0) {             // AMM_STOCK_LANGEVIN, operation by operation
                    const double g = amm_gaussian(A.seed, A.counter, (unsigned)t);
                    const double av = D.a * vt;
                    const double bf = D.b * ft;
                    const double drift = av + bf / m;
                    const double var = D.kT * (1.0 - D.a * D.a);
                    const double amp = sqrt(var / m);
                    w[k][j] = drift + amp * g;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (ms[k] > 0.0) {
                    const double dx = dt * w[k][j];
                    p[k][j] = x0[k][j] + dx;
                }
                if (dk[k] >= 0 && md[k] > 0.0) {
                    const double dx = dt * wd[k][j];
                    pd[k][j] = xd0[k][j] + dx;
                }
            }
        }
    }
    if constexpr (!std::is_same<S, ConsShapeNone>::value)
        if (!amm_shake_sweeps(s, p, x0, im, A.tol)) *A.fail = 1;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
            const int i = idx[k], dr = dk[k];
            const double m2 = ms[k], m1 = md[k];
            double vn[3], vq[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double dx = p[k][j] - x0[k][j];
                vn[j] = dx / dt;
                if (dr >= 0) {
                    const double dq = pd[k][j] - xd0[k][j];
                    vq[j] = dq / dt;
                }
            }
            if (dr >= 0 && m1 > 0.0 && D.wall > 0.0) {
                double d[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) d[j] = pd[k][j] - p[k][j];
                const double r = sqrt(dot3(d, d));
                if (r > 2.0 * D.wall) {
                    *A.flag = 1;
                } else if (r > D.wall) {
                    const double delta = r - D.wall;
                    double nh[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) nh[j] = d[j] / r;
                    double wp = dot3(vq, nh), w1 = dot3(vn, nh);
                    double rp[3], r1[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        rp[j] = vq[j] - wp * nh[j];
                        r1[j] = vn[j] - w1 * nh[j];
                    }
                    const double c = sqrt(D.kTD / m1);
                    if (m2 > 0.0) {
                        const double M = m1 + m2, f2 = m2 / M, f1 = m1 / M;
                        const double wbar = (m1 * wp + m2 * w1) / M;
                        wp -= wbar;
                        w1 -= wbar;
                        const double gap = fabs(wp - w1);
                        const double tau = gap > 0.0 ? fmin(dt, delta / gap) : dt;
                        wp = -copysign(1.0, wp) * c * f2;
                        w1 = -copysign(1.0, w1) * c * f1;
                        const double sp = -delta * f2 + tau * wp, s1 = delta * f1 + tau * w1;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            pd[k][j] += nh[j] * sp;
                            p[k][j] += nh[j] * s1;
                        }
                        wp += wbar;
                        w1 += wbar;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            vq[j] = rp[j] + wp * nh[j];
                            vn[j] = r1[j] + w1 * nh[j];
                        }
                    } else {
                        const double gap = fabs(wp);
                        const double tau = gap > 0.0 ? fmin(dt, delta / gap) : dt;
                        wp = -copysign(1.0, wp) * c;
                        const double sp = -delta + tau * wp;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            pd[k][j] += nh[j] * sp;
                            vq[j] = rp[j] + wp * nh[j];
                        }
                    }
                }
            }
            if (m2 > 0.0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int t = 3 * i + j;
                    A.x[t] = p[k][j];
                    A.v[t] = vn[j];
                    if (A.xref) A.xref[t] = p[k][j];
                }
                amm_watch_atom(A.W, i, p[k]);
            }
            if (dr >= 0 && m1 > 0.0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int t = 3 * dr + j;
                    A.x[t] = pd[k][j];
                    A.v[t] = vq[j];
                    if (A.xref) A.xref[t] = pd[k][j];
                }
                amm_watch_atom(A.W, dr, pd[k]);
            }
        }
    }
}

// GEN: the constraint set has clusters that are neither triangles nor pairs
template <bool GEN>
__global__ void __launch_bounds__(256) k_drude_step(DrudeStepArgs A) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= A.total) return;
    if (u < A.o_two) {
        if (u >= A.n_tri) return;
        const int c = A.units[u];
        const int idx[3] = {A.fixed[3 * u], A.fixed[3 * u + 1], A.fixed[3 * u + 2]};
        const ConsShapeTriangle S = {A.dist + A.cptr[c]};
        drude_unit(A, S, idx, 3);
    } else if (u < A.o_gen) {
        const int q = u - A.o_two;
        if (q >= A.n_two) return;
        const int c = A.units[A.n_tri + q];
        const int idx[2] = {A.fixed[3 * A.n_tri + 2 * q], A.fixed[3 * A.n_tri + 2 * q + 1]};
        const ConsShapePair S = {A.dist + A.cptr[c]};
        drude_unit(A, S, idx, 2);
    } else if (u < A.o_free) {
        if constexpr (GEN) {
            const int q = u - A.o_gen;
            if (q >= A.n_gen) return;
            const int c = A.units[A.n_tri + A.n_two + q], a0 = A.aptr[c], na = A.aptr[c + 1] - a0, c0 = A.cptr[c];
            int idx[AMM_CLUSTER_ATOMS];
#pragma unroll
            for (int k = 0; k < AMM_CLUSTER_ATOMS; ++k) idx[k] = k < na ? A.atoms[a0 + k] : 0;
            const ConsShapeGeneric S = {A.cptr[c + 1] - c0, A.pair + c0, A.dist + c0};
            drude_unit(A, S, idx, na);
        }
    } else {
        const int q = u - A.o_free;
        if (q >= A.n_free) return;
        const int idx[1] = {A.units ? A.units[A.n_tri + A.n_two + A.n_gen + q] : q};
        if (A.parent_of[idx[0]] >= 0) return;                                       // a Drude particle: its parent's unit moves it
        if (A.mass[idx[0]] == 0.0 && A.drude_of[idx[0]] < 0) return;                // a massless particle stores nothing
        drude_unit(A, ConsShapeNone(), idx, 1);
    }
}

int amm_drude_step_impl(amm_ctx *ctx, const DrudeStepDef &D, const double *d_f, unsigned long long counter) {
    const ConstraintSet *cs = ctx->constraints;
    DrudeStepArgs A = {};
    auto up64 = [](int k) { return (k + 63) / 64 * 64; };
    if (cs) {
        A.n_tri = cs->n_tri;
        A.n_two = cs->n_two;
        A.n_gen = cs->n_gen;
        A.n_free = cs->n_free;
        A.units = cs->d_units;
        A.fixed = cs->d_fixed;
        A.cptr = cs->d_cptr;
        A.aptr = cs->d_aptr;
        A.atoms = cs->d_atoms;
        A.pair = cs->d_pair;
        A.dist = cs->d_dist;
        A.tol = cs->tol;
        A.fail = cs->d_fail;
        A.xref = cs->d_xref;
    } else {
        A.n_free = ctx->n;
    }
    A.o_two = up64(A.n_tri);
    A.o_gen = A.o_two + up64(A.n_two);
    A.o_free = A.o_gen + up64(A.n_gen);
    A.total = A.o_free + A.n_free;
    A.x = ctx->d_x;
    A.v = ctx->d_v;
    A.f = d_f;
    A.mass = ctx->d_mass;
    A.drude_of = D.d_drude_of;
    A.parent_of = D.d_parent_of;
    A.flag = D.d_flag;
    A.D = D;
    A.seed = ctx->expr_seed;
    A.counter = counter;
    amm_collect_watches(ctx, A.W);           // (the caller bumps pos_epoch and calls amm_watch_moved)
    if (A.total <= 0) return 0;
    const dim3 grid((A.total + 255) / 256), block(256);
    if (A.n_gen > 0) hipLaunchKernelGGL(k_drude_step<true>, grid, block, 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_drude_step<false>, grid, block, 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    return 0;
}

int amm_drude_step_define_impl(amm_ctx *ctx, const int32_t *h_pairs, int n_pairs, double dt, double friction, double kT, double drude_friction,
                               double drude_kT, double max_distance, int *id) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_drude_step_define: " + what);
        return 1;
    };
    const int n = ctx->n;
    if (n_pairs < 0) return fail("a negative count");
    if (!(friction >= 0.0) || !(kT >= 0.0) || !(drude_friction >= 0.0) || !(drude_kT >= 0.0)) return fail("the frictions and kT must not be negative");
    if (!(dt == dt) || dt == 0.0) return fail("the step size must not be 0 (the velocities are differences of positions over it)");
    if (!(max_distance >= 0.0)) return fail("the hard wall distance must not be negative");
    if (ctx->world > 1) return fail("the Drude step runs on a single rank");
    std::vector<int> drude_of(n, -1), parent_of(n, -1);
    for (int k = 0; k < n_pairs; ++k) {
        const int p = h_pairs[2 * k], p1 = h_pairs[2 * k + 1];
        if (p < 0 || p >= n || p1 < 0 || p1 >= n || p == p1) return fail("pair " + std::to_string(k) + " names a particle out of range, or one twice");
        if (drude_of[p] >= 0 || parent_of[p] >= 0 || drude_of[p1] >= 0 || parent_of[p1] >= 0)
            return fail("pair " + std::to_string(k) + " names a particle that another pair names");
        drude_of[p1] = p;
        parent_of[p] = p1;
    }
    AMM_HIP(hipSetDevice(ctx->device));
    DrudeStepDef D;
    D.dt = dt;
    D.kT = kT;
    D.kTD = drude_kT;
    D.a = exp(-friction * dt);
    D.b = friction > 0.0 ? (1.0 - D.a) / friction : dt;
    D.aD = exp(-drude_friction * dt);
    D.bD = drude_friction > 0.0 ? (1.0 - D.aD) / drude_friction : dt;
    D.wall = max_distance;
    D.n_pairs = n_pairs;
    if (amm_upload(&D.d_drude_of, drude_of.data(), drude_of.size())) return 1;
    if (amm_upload(&D.d_parent_of, parent_of.data(), parent_of.size())) return 1;
    AMM_HIP(hipMalloc(&D.d_flag, sizeof(int)));
    AMM_HIP(hipMemset(D.d_flag, 0, sizeof(int)));
    ctx->drude_steps.push_back(D);
    *id = (int)ctx->drude_steps.size() - 1;
    return 0;
}

// 1: a pair went beyond twice the hard wall since the last call (the flag is cleared); -1: the read failed
int amm_drude_step_flagged(amm_ctx *ctx) {
    int any = 0;
    for (DrudeStepDef &D : ctx->drude_steps) {
        int flag = 0;
        if (hipMemcpy(&flag, D.d_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (flag) {
            (void)hipMemset(D.d_flag, 0, sizeof(int));
            any = 1;
        }
    }
    return any;
}

void amm_drude_steps_free(amm_ctx *ctx) {
    for (DrudeStepDef &D : ctx->drude_steps)
        for (void *p : {(void *)D.d_drude_of, (void *)D.d_parent_of, (void *)D.d_flag})
            if (p) (void)hipFree(p);
    ctx->drude_steps.clear();
}
