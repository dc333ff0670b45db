// atomsmm_amd/csrc/rmsd_fit.h -- the rigid fit of rmsd.hip: from the twelve sums of a selection (sum x, sum y' (x) x with the reference
// y' centred) the centroid c of the positions and the proper rotation R that minimises sum |x - c - R y'|^2 (Horn 1987: R is the
// rotation of the unit quaternion that is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix N built from M).
// Host and device: the device runs it on one lane, a host program can run the same arithmetic.
#pragma once

#ifndef AMM_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMM_HD __host__ __device__
#else
#define AMM_HD
#endif
#endif

#define AMM_RMSD_SWEEPS 12      // cyclic Jacobi sweeps over the six off-diagonal pairs at the most: a 4 x 4 matrix is diagonal to rounding
                                // after five or six, and the sweep that finds every rotation negligible ends the iteration

#if defined(__HIP_DEVICE_COMPILE__)
#define AMM_RMSD_RSQRT(x) rsqrt(x)
#else
#define AMM_RMSD_RSQRT(x) (1.0 / sqrt(x))
#endif

// One Jacobi rotation in the (P, Q) plane of the symmetric matrix a (kept in full storage), accumulated in v; returns whether it
// rotated.  A rotation whose off-diagonal element is zero, or so small that adding it changes neither diagonal element, is skipped
// (the element is cleared): the textbook theta = (a_qq - a_pp) / (2 a_pq) would overflow there.  The tangent of the smaller angle
// is taken in the form that needs no theta, t = sgn(d) b / (|d| + sqrt(d^2 + b^2)) with d = a_qq - a_pp and b = 2 a_pq: one square
// root and one division, nothing to overflow for a small b; a denominator of zero (d = 0 and b^2 underflowed) is the 45 degree
// rotation, and |t| <= 1 is enforced, so that c and s are finite whatever the squares did -- never a NaN.  The fp64 division and
// square root are some tens of dependent instructions each on one lane: three of them per rotation, where the textbook has five.
template <int P, int Q>
AMM_HD inline bool amm_rmsd_rotate(double (&a)[4][4], double (&v)[4][4]) {
#pragma clang fp contract(off)
    const double apq = a[P][Q];
    const double g = apq < 0.0 ? -apq : apq;
    if (g == 0.0) return false;
    const double app = a[P][P], aqq = a[Q][Q];
    const double dp = app < 0.0 ? -app : app, dq = aqq < 0.0 ? -aqq : aqq;
    if (dp + g == dp && dq + g == dq) {
        a[P][Q] = 0.0;
        a[Q][P] = 0.0;
        return false;
    }
    const double d = aqq - app, b = 2.0 * apq;
    const double ad = d < 0.0 ? -d : d;
    const double den = ad + sqrt(d * d + b * b);
    double t = den > 0.0 ? b / den : 1.0;
    if (d < 0.0) t = -t;
    t = t > 1.0 ? 1.0 : (t < -1.0 ? -1.0 : t);
    const double c = AMM_RMSD_RSQRT(t * t + 1.0), s = t * c;
    const double h = t * apq;
    a[P][P] = app - h;
    a[Q][Q] = aqq + h;
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = a[k][P], akq = a[k][Q];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            a[k][P] = np;
            a[P][k] = np;
            a[k][Q] = nq;
            a[Q][k] = nq;
        }
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
    return true;
}

// sums[0..2] = sum x, sums[3 + 3 a + b] = sum y'_a x_b over the n_sel particles; fit[0..2] = c, fit[3 + 3 a + b] = R_ab
AMM_HD inline void amm_rmsd_fit(const double *sums, int n_sel, double *fit) {
#pragma clang fp contract(off)
    const double inv_n = 1.0 / (double)n_sel;
    fit[0] = sums[0] * inv_n;
    fit[1] = sums[1] * inv_n;
    fit[2] = sums[2] * inv_n;
    const double Sxx = sums[3], Sxy = sums[4], Sxz = sums[5], Syx = sums[6], Syy = sums[7], Syz = sums[8], Szx = sums[9], Szy = sums[10],
                 Szz = sums[11];
    double a[4][4], v[4][4];
    a[0][0] = Sxx + Syy + Szz;
    a[1][1] = Sxx - Syy - Szz;
    a[2][2] = -Sxx + Syy - Szz;
    a[3][3] = -Sxx - Syy + Szz;
    a[0][1] = a[1][0] = Syz - Szy;
    a[0][2] = a[2][0] = Szx - Sxz;
    a[0][3] = a[3][0] = Sxy - Syx;
    a[1][2] = a[2][1] = Sxy + Syx;
    a[1][3] = a[3][1] = Szx + Sxz;
    a[2][3] = a[3][2] = Syz + Szy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < AMM_RMSD_SWEEPS; ++sweep) {
        bool rotated = amm_rmsd_rotate<0, 1>(a, v);
        rotated |= amm_rmsd_rotate<0, 2>(a, v);
        rotated |= amm_rmsd_rotate<0, 3>(a, v);
        rotated |= amm_rmsd_rotate<1, 2>(a, v);
        rotated |= amm_rmsd_rotate<1, 3>(a, v);
        rotated |= amm_rmsd_rotate<2, 3>(a, v);
        if (!rotated) break;           // (every off-diagonal element is negligible: further sweeps would skip the same six)
    }
    // the column of the largest eigenvalue (the first of equal ones: any unit vector of a degenerate top eigenspace gives the same residual)
    double q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0], top = a[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > top) {
            top = a[k][k];
            q0 = v[0][k];
            q1 = v[1][k];
            q2 = v[2][k];
            q3 = v[3][k];
        }
    const double norm = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);      // (v is orthogonal to rounding: the norm is 1 - O(eps))
    q0 *= norm;
    q1 *= norm;
    q2 *= norm;
    q3 *= norm;
    fit[3] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
    fit[4] = 2.0 * (q1 * q2 - q0 * q3);
    fit[5] = 2.0 * (q1 * q3 + q0 * q2);
    fit[6] = 2.0 * (q1 * q2 + q0 * q3);
    fit[7] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
    fit[8] = 2.0 * (q2 * q3 - q0 * q1);
    fit[9] = 2.0 * (q1 * q3 - q0 * q2);
    fit[10] = 2.0 * (q2 * q3 + q0 * q1);
    fit[11] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}
