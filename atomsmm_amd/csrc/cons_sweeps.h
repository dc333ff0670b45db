// atomsmm_amd/csrc/cons_sweeps.h -- the constraint set of a context and the Gauss-Seidel sweeps of its solvers (SHAKE on positions,
// RATTLE on velocities), shared by the stand-alone kernels k_shake / k_rattle (constraints.hip) and the one-launch stock-integrator
// step (stock.hip).  See constraints.hip for the semantics.
//
// A sweep walks a cluster's constraints in their order.  WHICH constraints a cluster has is a "shape": the generic shape reads the
// (i, j) pairs from memory and indexes the cluster's private arrays at run time (which this compiler keeps in scratch memory); the
// rigid three-site triangle and the two-atom pair are shapes whose indices are compile-time constants, so that after unrolling
// every array element is a register.
#pragma once
#include "amm_ctx.h"

#define AMM_CLUSTER_CONS 16
#define AMM_CONS_SWEEPS 500

// classes of a cluster: decided once, when the set is created (amm_constraints_create_impl)
enum : int { AMM_CONS_GENERIC = 0, AMM_CONS_TRIANGLE = 1, AMM_CONS_PAIR = 2 };

struct ConstraintSet {
    int ncluster = 0;
    double tol = 1e-5;
    int *d_cptr = nullptr;       // [ncluster+1] constraints of each cluster
    int *d_aptr = nullptr;       // [ncluster+1] atoms of each cluster
    int *d_atoms = nullptr;      // atom indices, cluster by cluster
    int2 *d_pair = nullptr;      // constraint -> (local i, local j) within its cluster
    double *d_dist = nullptr;    // constraint -> distance
    double *d_xref = nullptr;    // [n][3] reference positions (see above)
    int *d_fail = nullptr;       // set when a cluster does not converge
    // work units of the stock-integrator step (stock.hip): the clusters by class -- triangles (three atoms, each pair of them
    // constrained), pairs (two atoms, one constraint), everything else -- and the atoms that belong to no cluster
    int n_tri = 0, n_two = 0, n_gen = 0, n_free = 0;
    int *d_units = nullptr;      // [n_tri + n_two + n_gen] cluster indices, class by class; then [n_free] atom indices
    // the atoms of the triangles [n_tri][3] and then of the pairs [n_two][2], each cluster's in the order in which its constraints,
    // walked in their order, read (0,1), (0,2), (1,2) / (0,1).  (Which end of a constraint is i and which j does not matter: every
    // term of a sweep changes sign twice or not at all, so the results are the same bit for bit.)
    int *d_fixed = nullptr;
};

struct ConsArgs {
    int ncluster;
    const int *cptr, *aptr, *atoms;
    const int2 *pair;
    const double *dist;
    const double *mass;
    double tol;
    int *fail;
};

// ---- shapes: n() constraints, constraint q couples local atoms ij(q) at distance d(q) ----
struct ConsShapeGeneric {
    static constexpr int NA = AMM_CLUSTER_ATOMS;
    int nc;
    const int2 *pair;
    const double *dist;
    __device__ __forceinline__ int n() const { return nc; }
    __device__ __forceinline__ int2 ij(int q) const { return pair[q]; }
    __device__ __forceinline__ double d(int q) const { return dist[q]; }
};
struct ConsShapeTriangle {
    static constexpr int NA = 3;
    const double *dist;
    __device__ __forceinline__ constexpr int n() const { return 3; }
    __device__ __forceinline__ int2 ij(int q) const { return q == 0 ? make_int2(0, 1) : q == 1 ? make_int2(0, 2) : make_int2(1, 2); }
    __device__ __forceinline__ double d(int q) const { return dist[q]; }
};
struct ConsShapePair {
    static constexpr int NA = 2;
    const double *dist;
    __device__ __forceinline__ constexpr int n() const { return 1; }
    __device__ __forceinline__ int2 ij(int) const { return make_int2(0, 1); }
    __device__ __forceinline__ double d(int q) const { return dist[q]; }
};
struct ConsShapeNone {       // an atom in no cluster
    static constexpr int NA = 1;
    __device__ __forceinline__ constexpr int n() const { return 0; }
    __device__ __forceinline__ int2 ij(int) const { return make_int2(0, 0); }
    __device__ __forceinline__ double d(int) const { return 0.0; }
};

// SHAKE: positions p onto the constraint surface along the bond vectors of the reference positions r; false: not converged
template <class S, int NA>
__device__ __forceinline__ bool amm_shake_sweeps(const S &s, double (&p)[NA][3], const double (&r)[NA][3], const double (&im)[NA],
                                                 double tol) {
    const double lower = 1.0 - 2.0 * tol + tol * tol, upper = 1.0 + 2.0 * tol + tol * tol;
    const int nc = s.n();
    bool done = false;
    for (int it = 0; it < AMM_CONS_SWEEPS && !done; ++it) {
        done = true;
        for (int q = 0; q < nc; ++q) {       // (a fixed shape: a constant trip count, unrolled in full)
            const int2 ij = s.ij(q);
            const double dq = s.d(q);
            const double d2 = dq * dq;
            double dp[3], dr[3], pp = 0.0, rp = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dp[j] = p[ij.x][j] - p[ij.y][j];
                dr[j] = r[ij.x][j] - r[ij.y][j];
                pp += dp[j] * dp[j];
                rp += dr[j] * dp[j];
            }
            // (negated, so that a NaN also counts as "not there yet": a cluster that is not finite runs out of sweeps and fails)
            if (!(pp >= lower * d2 && pp <= upper * d2)) {
                done = false;
                const double g = (d2 - pp) / (2.0 * (im[ij.x] + im[ij.y]) * rp);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    p[ij.x][j] += g * im[ij.x] * dr[j];
                    p[ij.y][j] -= g * im[ij.y] * dr[j];
                }
            }
        }
    }
    return done;
}

// RATTLE: remove from the velocities w the components along the constrained bonds of the positions p; false: not converged
template <class S, int NA>
__device__ __forceinline__ bool amm_rattle_sweeps(const S &s, const double (&p)[NA][3], double (&w)[NA][3], const double (&im)[NA],
                                                  double tol) {
    const int nc = s.n();
    bool done = false;
    for (int it = 0; it < AMM_CONS_SWEEPS && !done; ++it) {
        done = true;
        for (int q = 0; q < nc; ++q) {       // (a fixed shape: a constant trip count, unrolled in full)
            const int2 ij = s.ij(q);
            double dp[3], dot = 0.0, pp = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dp[j] = p[ij.x][j] - p[ij.y][j];
                dot += dp[j] * (w[ij.x][j] - w[ij.y][j]);
                pp += dp[j] * dp[j];
            }
            // relative rate of change of the bond length, d ln|r| / dt, against the tolerance (1/ps); negated: NaN also triggers
            if (!(fabs(dot) <= tol * pp)) {
                done = false;
                const double g = -dot / ((im[ij.x] + im[ij.y]) * pp);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    w[ij.x][j] += g * im[ij.x] * dp[j];
                    w[ij.y][j] -= g * im[ij.y] * dp[j];
                }
            }
        }
    }
    return done;
}
