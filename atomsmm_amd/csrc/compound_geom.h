// atomsmm_amd/csrc/compound_geom.h -- one geometric variable of a compound-bond text and its gradient on its roles: what k_compound
// (compound.hip) computes per (bond, variable) and k_hbond (hbond.hip) per (surviving pair, variable).  The geometry is that of
// k_term_expr (term_expr.hip): delta3 / cross3 / amm_min_image of bonded_terms.h, the angle gradient with its 1 - c^2 floor, the
// dihedral convention and gradient of AMM_TORSION_PERIODIC.
#pragma once
#include "amm_ctx.h"
#include "bonded_terms.h"

#ifdef __HIPCC__
// kind: AMM_CVAR_*; a0 .. a3: the atoms (or centres) of the variable's roles (any valid index behind its arity).  Leaves the value in
// v and grad v on role r in gr -- for a distance the UNNORMALISED displacement, with rr = r for the caller to divide the coefficient
// by (rr = 1 otherwise).  g0 .. g3 come in zeroed; the roles behind the arity stay so.
template <class P>
__device__ __forceinline__ void compound_variable(const P &pos, int kind, int a0, int a1, int a2, int a3, const Box &box, int periodic,
                                                  double &v, double &rr, double *g0, double *g1, double *g2, double *g3) {
#pragma clang fp contract(off)
    if (kind <= AMM_CVAR_Z) {               // a raw coordinate: never wrapped
        v = pos.get(a0, kind);
        g0[0] = kind == AMM_CVAR_X ? 1.0 : 0.0;
        g0[1] = kind == AMM_CVAR_Y ? 1.0 : 0.0;
        g0[2] = kind == AMM_CVAR_Z ? 1.0 : 0.0;
    } else if (kind == AMM_CVAR_DISTANCE) {
        double d[3];
        delta3(pos, a0, a1, box, periodic, d);
        rr = sqrt(dot3(d, d));
        v = rr;
#pragma unroll
        for (int x = 0; x < 3; ++x) {       // (grad r = d / r: the division goes into the coefficient, as k_term_expr has it)
            g0[x] = d[x];
            g1[x] = -d[x];
        }
    } else if (kind == AMM_CVAR_ANGLE) {
        double d1[3], d2[3];
        delta3(pos, a0, a1, box, periodic, d1);
        delta3(pos, a2, a1, box, periodic, d2);
        const double i1 = amm_rsqrt(dot3(d1, d1)), i2 = amm_rsqrt(dot3(d2, d2));
        double c = dot3(d1, d2) * i1 * i2;
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        v = acos(c);
        double s2 = 1.0 - c * c;
        if (s2 < 1e-24) s2 = 1e-24;
        const double rs = amm_rsqrt(s2);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double u1 = d1[x] * i1, u2 = d2[x] * i2;      // unit vectors
            const double gi = -(rs * (u2 - c * u1) * i1);
            const double gk = -(rs * (u1 - c * u2) * i2);
            g0[x] = gi;
            g1[x] = -(gi + gk);
            g2[x] = gk;
        }
    } else {                                // AMM_CVAR_DIHEDRAL
        double F[3], G[3], H[3], Av[3], Bv[3], BA[3];
        delta3(pos, a0, a1, box, periodic, F);
        delta3(pos, a1, a2, box, periodic, G);
        delta3(pos, a3, a2, box, periodic, H);
        cross3(F, G, Av);
        cross3(H, G, Bv);
        cross3(Bv, Av, BA);
        const double Gn = sqrt(dot3(G, G));
        v = atan2(dot3(BA, G) / Gn, dot3(Av, Bv));
        const double A2 = dot3(Av, Av), B2 = dot3(Bv, Bv), FG = dot3(F, G), HG = dot3(H, G);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            g0[x] = -Gn / A2 * Av[x];
            g1[x] = Gn / A2 * Av[x] + FG / (A2 * Gn) * Av[x] - HG / (B2 * Gn) * Bv[x];
            g2[x] = -Gn / B2 * Bv[x] - FG / (A2 * Gn) * Av[x] + HG / (B2 * Gn) * Bv[x];
            g3[x] = Gn / B2 * Bv[x];
        }
    }
}

// The tail of a drain: the `take` entries at the front of the queue are done, what is left (fewer than 64) moves to the front.
// Every lane of the block (one wavefront) reaches the two barriers.  Returns the entries left.
template <class T>
__device__ __forceinline__ int queue_keep_rest(T *s_queue, int qn, int take) {
    const int rest = qn - take;
    const T moved = (int)threadIdx.x < rest ? s_queue[AMM_WAVE + threadIdx.x] : T{};
    __syncthreads();
    if ((int)threadIdx.x < rest) s_queue[threadIdx.x] = moved;
    __syncthreads();
    return rest;
}
#endif
