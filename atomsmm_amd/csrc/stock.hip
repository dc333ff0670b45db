// atomsmm_amd/csrc/stock.hip -- AMM_OP_STOCK: the whole post-force update of one step of OpenMM's stock integrators in ONE launch
// (gfx950, fp64).
//
// The formulas are those of OpenMM's Reference platform, restated [recalled -- OpenMM's sources are not at hand; as in
// constraints.hip].  With f the forces at x, m the mass, N a standard normal number per degree of freedom, a = exp(-friction dt):
//   0 Verlet (leapfrog)   v1 = v + dt f/m ; x' = x + dt v1 ; SHAKE x' along the bond vectors of x ; v = (x' - x)/dt
//   1 LangevinMiddle      v1 = v + dt f/m ; RATTLE v1 at x ; xh = x + dt/2 v1 ; v2 = a v1 + sqrt(kT (1 - a^2)/m) N ;
//                         x1 = xh + dt/2 v2 ; x' = SHAKE of x1 along the bond vectors of x ; v = v2 + (x' - x1)/dt
//   2 Langevin            v1 = a v + b f/m + sqrt(kT (1 - a^2)/m) N, b = (1 - a)/friction (dt when friction = 0) ; then as Verlet
//                         from x' = x + dt v1
//   3 Brownian            x' = x + (dt/friction) f/m + sqrt(2 kT dt/(friction m)) N ; SHAKE ; v = (x' - x)/dt
// N is amm_gaussian(seed, counter, dof) with one counter per op: the stream of AMM_OP_BATH / AMM_OP_EXPR, so that a step draws
// what the op-by-op program with one random op draws.  Every operation rounds as the separate ops round it (no contraction into
// FMA in the step arithmetic; the sweeps are the functions k_shake / k_rattle call).
//
// MI355X mapping: written op by op, a constrained Langevin-middle step is eight launches that stream x or v through HBM.  Here the
// work unit is a constraint cluster (or an atom of no cluster) and ONE THREAD carries its unit from the loads to the stores:
// 3 loads (x, v, f) and 2 or 3 stores (x, v, the solver's reference) per degree of freedom for the whole step.  The rigid three-site
// triangle and the two-atom pair have instantiations whose array indices are compile-time constants (cons_sweeps.h): every element
// is a register.  Other clusters take the generic sweep, whose run-time indices put the arrays in scratch memory; a constraint
// set without such clusters launches the instantiation without that path (no scratch at all).  Classes start at multiples of the
// wavefront size in the unit index space, so that a wavefront never holds two classes.
#include <type_traits>

#include "cons_sweeps.h"
#include "bonded_terms.h"
#include "expr_vm.h"

struct StockArgs {
    int n_tri, n_two, n_gen, n_free;       // units of each class
    int o_two, o_gen, o_free, total;       // where the classes start in the unit index space (multiples of 64)
    const int *units;                      // ConstraintSet::d_units; null: no constraint set -- free unit q is atom q
    const int *fixed;                      // ConstraintSet::d_fixed: the atoms of the triangles, then of the pairs
    const int *cptr, *aptr, *atoms;
    const int2 *pair;
    const double *dist;
    double tol;
    int *fail;
    double *x, *v, *xref;
    const double *f, *mass;
    StockDef sd;
    unsigned long long seed, counter;
    WatchArgs W;
};

// one unit: atoms idx[0 .. na) (na = S::NA for the fixed shapes)
template <class S>
__device__ __forceinline__ void stock_unit(const StockArgs &A, const S &s, const int (&idx)[S::NA], int na) {
#pragma clang fp contract(off)
    constexpr int NA = S::NA;
    const StockDef &D = A.sd;
    const double dt = D.dt;
    double x0[NA][3], p[NA][3], w[NA][3], im[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
            const int i = idx[k];
            const double m = A.mass[i];
            im[k] = 1.0 / m;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = 3 * i + j;
                const double xt = A.x[t], vt = A.v[t], ft = A.f[t];
                x0[k][j] = xt;
                if (D.kind == AMM_STOCK_VERLET || D.kind == AMM_STOCK_LANGEVIN_MIDDLE) {
                    const double num = dt * ft;                  // the kick v + (dt f)/m, as AMM_OP_KICK rounds it
                    const double dv = num / m;
                    w[k][j] = vt + dv;
                } else if (D.kind == AMM_STOCK_LANGEVIN) {
                    const double g = amm_gaussian(A.seed, A.counter, (unsigned)t);
                    const double av = D.a * vt;
                    const double bf = D.b * ft;
                    const double drift = av + bf / m;
                    const double var = D.kT * (1.0 - D.a * D.a);
                    const double amp = sqrt(var / m);
                    w[k][j] = drift + amp * g;
                } else {
                    w[k][j] = vt;                                // (Brownian: the velocities are what the step leaves)
                }
                p[k][j] = xt;
            }
        }
    }
    if (D.kind == AMM_STOCK_LANGEVIN_MIDDLE) {
        if constexpr (!std::is_same<S, ConsShapeNone>::value)
            if (!amm_rattle_sweeps(s, p, w, im, A.tol)) *A.fail = 1;
    }
    // the unconstrained new positions, in p; x1[k][j] keeps them for the middle scheme's velocity correction
    double x1[NA][3];
    const double hdt = 0.5 * dt;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
            const int i = idx[k];
            const double m = A.mass[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = 3 * i + j;
                if (D.kind == AMM_STOCK_LANGEVIN_MIDDLE) {
                    const double dxa = hdt * w[k][j];
                    const double xh = x0[k][j] + dxa;
                    w[k][j] = amm_ou_step(w[k][j], m, D.a, D.kT, amm_gaussian(A.seed, A.counter, (unsigned)t));
                    const double dxb = hdt * w[k][j];
                    p[k][j] = xh + dxb;
                } else if (D.kind == AMM_STOCK_BROWNIAN) {
                    const double g = amm_gaussian(A.seed, A.counter, (unsigned)t);
                    const double c = dt / D.friction;
                    const double s2 = 2.0 * D.kT * dt / D.friction;
                    const double cf = c * A.f[t];
                    const double drift = x0[k][j] + cf / m;
                    const double amp = sqrt(s2 / m);
                    p[k][j] = drift + amp * g;
                } else {
                    const double dx = dt * w[k][j];
                    p[k][j] = x0[k][j] + dx;
                }
                x1[k][j] = p[k][j];
            }
        }
    }
    if constexpr (!std::is_same<S, ConsShapeNone>::value)
        if (!amm_shake_sweeps(s, p, x0, im, A.tol)) *A.fail = 1;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k < na) {
            const int i = idx[k];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = 3 * i + j;
                double vn;
                if (D.kind == AMM_STOCK_LANGEVIN_MIDDLE) {
                    const double dx = p[k][j] - x1[k][j];
                    vn = w[k][j] + dx / dt;
                } else {
                    const double dx = p[k][j] - x0[k][j];
                    vn = dx / dt;
                }
                A.x[t] = p[k][j];
                A.v[t] = vn;
                if (A.xref) A.xref[t] = p[k][j];       // the constrained positions are the solver's next reference
            }
            amm_watch_atom(A.W, i, p[k]);
        }
    }
}

// GEN: the constraint set has clusters that are neither triangles nor pairs
template <bool GEN>
__global__ void __launch_bounds__(256) k_stock(StockArgs A) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= A.total) return;
    if (u < A.o_two) {
        if (u >= A.n_tri) return;
        const int c = A.units[u];
        const int idx[3] = {A.fixed[3 * u], A.fixed[3 * u + 1], A.fixed[3 * u + 2]};
        const ConsShapeTriangle S = {A.dist + A.cptr[c]};
        stock_unit(A, S, idx, 3);
    } else if (u < A.o_gen) {
        const int q = u - A.o_two;
        if (q >= A.n_two) return;
        const int c = A.units[A.n_tri + q];
        const int idx[2] = {A.fixed[3 * A.n_tri + 2 * q], A.fixed[3 * A.n_tri + 2 * q + 1]};
        const ConsShapePair S = {A.dist + A.cptr[c]};
        stock_unit(A, S, idx, 2);
    } else if (u < A.o_free) {
        if constexpr (GEN) {
            const int q = u - A.o_gen;
            if (q >= A.n_gen) return;
            const int c = A.units[A.n_tri + A.n_two + q], a0 = A.aptr[c], na = A.aptr[c + 1] - a0, c0 = A.cptr[c];
            int idx[AMM_CLUSTER_ATOMS];
#pragma unroll
            for (int k = 0; k < AMM_CLUSTER_ATOMS; ++k) idx[k] = k < na ? A.atoms[a0 + k] : 0;
            const ConsShapeGeneric S = {A.cptr[c + 1] - c0, A.pair + c0, A.dist + c0};
            stock_unit(A, S, idx, na);
        }
    } else {
        const int q = u - A.o_free;
        if (q >= A.n_free) return;
        const int idx[1] = {A.units ? A.units[A.n_tri + A.n_two + A.n_gen + q] : q};
        if (A.mass[idx[0]] == 0.0) return;       // a massless particle (a virtual site; never in a cluster) stores nothing
        stock_unit(A, ConsShapeNone(), idx, 1);
    }
}

int amm_stock_step_impl(amm_ctx *ctx, const StockDef &sd, const double *d_f, unsigned long long counter) {
    const ConstraintSet *cs = ctx->constraints;
    StockArgs A = {};
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
    A.sd = sd;
    A.seed = ctx->expr_seed;
    A.counter = counter;
    amm_collect_watches(ctx, A.W);           // (the caller bumps pos_epoch and calls amm_watch_moved)
    if (A.total <= 0) return 0;
    const dim3 grid((A.total + 255) / 256), block(256);
    if (A.n_gen > 0) hipLaunchKernelGGL(k_stock<true>, grid, block, 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_stock<false>, grid, block, 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    return 0;
}
