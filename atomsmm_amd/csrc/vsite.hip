// atomsmm_amd/csrc/vsite.hip -- virtual sites: massless particles whose positions are functions of up to three parents (gfx950, fp64).
//
// OpenMM's TwoParticleAverageSite, ThreeParticleAverageSite and OutOfPlaneSite [formulas as OpenMM's ReferenceVirtualSites takes them,
// restated: plain differences of the parents' positions -- the parents of a site belong to one molecule and molecules are never split
// across the box]:
//   average2 / average3   s = w1 r1 + w2 r2 [+ w3 r3]                                   f_k += w_k f
//   outOfPlane            s = r1 + w12 r12 + w13 r13 + wc (r12 x r13)                   f2 += w12 f + wc (r13 x f)
//                         r12 = r2 - r1, r13 = r3 - r1                                  f3 += w13 f + wc (f x r12)
//                                                                                       f1 += f - (the f2 and f3 parts)
// amm_vsite_place writes the sites' positions from their parents'; amm_vsite_spread hands the force a site collected to its parents
// (J^T f) and zeroes the site's row, so that what integrates the massive atoms sees the whole force and the sites none.
//
// MI355X mapping: both are latency bound (a few hundred to a few ten thousand items, tens of bytes each).  Place: one lane per site,
// launched over the sites only.  Spread: owner-computes like the bond lists -- the host builds a CSR parent atom -> its (site, role)
// entries sorted by site, one lane per parent atom WITH entries adds them in that order into its own row: no atomics, the same bits
// from run to run whatever number of sites an atom carries.  The sites' rows are zeroed by a second launch: in the same grid a lane
// that zeroes a row would race with the parents' lanes that still read it.  No LDS; 256-thread blocks sized by the item count.
// Every operation rounds on its own (no contraction into FMA), so that the numpy restatement of the tests rounds identically.
#include <algorithm>
#include <cmath>

#include "amm_ctx.h"

#pragma clang fp contract(off)

struct VsiteSet {
    int n_sites = 0, n_owners = 0;
    int *d_site = nullptr, *d_kind = nullptr, *d_parents = nullptr;     // [n_sites], [n_sites], [n_sites][3]
    double *d_weights = nullptr;                                         // [n_sites][3]
    int *d_owner = nullptr, *d_optr = nullptr, *d_oent = nullptr;        // parent atoms with entries; CSR; entry = site index * 4 + role
    long long n_place = 0, n_spread = 0, n_launches = 0;
};

struct VsiteArgs {
    int n_sites, n_owners;
    const int *site, *kind, *parents, *owner, *optr, *oent;
    const double *weights;
};

__device__ __forceinline__ void vs_load(const double *x, int i, double (&r)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = x[3 * (size_t)i + k];
}
__device__ __forceinline__ void vs_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    const double p0 = a[1] * b[2], q0 = a[2] * b[1], p1 = a[2] * b[0], q1 = a[0] * b[2], p2 = a[0] * b[1], q2 = a[1] * b[0];
    c[0] = p0 - q0;
    c[1] = p1 - q1;
    c[2] = p2 - q2;
}

__global__ void __launch_bounds__(256) k_vsite_place(VsiteArgs A, double *x) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.n_sites) return;
    const int kind = A.kind[s], p1 = A.parents[3 * s], p2 = A.parents[3 * s + 1], p3 = A.parents[3 * s + 2];
    const double w0 = A.weights[3 * s], w1 = A.weights[3 * s + 1], w2 = A.weights[3 * s + 2];
    double r1[3], r2[3], r3[3] = {0.0, 0.0, 0.0}, out[3];
    vs_load(x, p1, r1);
    vs_load(x, p2, r2);
    if (kind != AMM_VSITE_AVERAGE2) vs_load(x, p3, r3);
    if (kind == AMM_VSITE_OUT_OF_PLANE) {
        double r12[3], r13[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r12[k] = r2[k] - r1[k];
            r13[k] = r3[k] - r1[k];
        }
        vs_cross(r12, r13, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = w0 * r12[k], b = w1 * r13[k], d = w2 * c[k];
            out[k] = ((r1[k] + a) + b) + d;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = w0 * r1[k], b = w1 * r2[k];
            double sum = a + b;
            if (kind == AMM_VSITE_AVERAGE3) {
                const double d = w2 * r3[k];
                sum = sum + d;
            }
            out[k] = sum;
        }
    }
    const size_t o = 3 * (size_t)A.site[s];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[o + k] = out[k];
}

// the share of parent `role` (0, 1, 2) in the force f on site s
__device__ __forceinline__ void vs_share(const VsiteArgs &A, const double *x, int s, int role, const double (&f)[3], double (&g)[3]) {
    const int kind = A.kind[s];
    if (kind != AMM_VSITE_OUT_OF_PLANE) {
        const double w = A.weights[3 * s + role];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = w * f[k];
        return;
    }
    const double w12 = A.weights[3 * s], w13 = A.weights[3 * s + 1], wc = A.weights[3 * s + 2];
    double r1[3], r2[3], r3[3], r12[3], r13[3], c2[3], c3[3], f2[3], f3[3];
    vs_load(x, A.parents[3 * s], r1);
    vs_load(x, A.parents[3 * s + 1], r2);
    vs_load(x, A.parents[3 * s + 2], r3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r12[k] = r2[k] - r1[k];
        r13[k] = r3[k] - r1[k];
    }
    vs_cross(r13, f, c2);
    vs_cross(f, r12, c3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a2 = w12 * f[k], b2 = wc * c2[k], a3 = w13 * f[k], b3 = wc * c3[k];
        f2[k] = a2 + b2;
        f3[k] = a3 + b3;
        g[k] = role == 1 ? f2[k] : role == 2 ? f3[k] : (f[k] - f2[k]) - f3[k];
    }
}

// one lane per parent atom that carries sites: its entries in the order of the sites
__global__ void __launch_bounds__(256) k_vsite_spread(VsiteArgs A, const double *x, double *f) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n_owners) return;
    const size_t o = 3 * (size_t)A.owner[q];
    double acc[3] = {f[o], f[o + 1], f[o + 2]};
    for (int e = A.optr[q]; e < A.optr[q + 1]; ++e) {
        const int ent = A.oent[e], s = ent >> 2, role = ent & 3;
        double fs[3], g[3];
        vs_load(f, A.site[s], fs);
        vs_share(A, x, s, role, fs, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + g[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) f[o + k] = acc[k];
}
__global__ void __launch_bounds__(256) k_vsite_zero(VsiteArgs A, double *f) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.n_sites) return;
    const size_t o = 3 * (size_t)A.site[s];
    f[o] = 0.0;
    f[o + 1] = 0.0;
    f[o + 2] = 0.0;
}

static void vsite_args(const VsiteSet *vs, VsiteArgs &A) {
    A.n_sites = vs->n_sites;
    A.n_owners = vs->n_owners;
    A.site = vs->d_site;
    A.kind = vs->d_kind;
    A.parents = vs->d_parents;
    A.owner = vs->d_owner;
    A.optr = vs->d_optr;
    A.oent = vs->d_oent;
    A.weights = vs->d_weights;
}

int amm_vsite_free(amm_ctx *ctx) {
    VsiteSet *vs = ctx->vsites;
    if (!vs) return 0;
    for (int **p : {&vs->d_site, &vs->d_kind, &vs->d_parents, &vs->d_owner, &vs->d_optr, &vs->d_oent})
        if (*p) (void)hipFree(*p);
    if (vs->d_weights) (void)hipFree(vs->d_weights);
    delete vs;
    ctx->vsites = nullptr;
    return 0;
}

int amm_vsite_define_impl(amm_ctx *ctx, int n_sites, const int32_t *h_site, const int32_t *h_kind, const int32_t *h_parents,
                          const double *h_weights) {
    const int n = ctx->n;
    std::vector<char> is_site((size_t)n, 0);
    for (int s = 0; s < n_sites; ++s) {
        const int i = h_site[s];
        if (i < 0 || i >= n || is_site[i]) {
            amm_set_error("amm_vsite_define: site " + std::to_string(s) + " is atom " + std::to_string(i) +
                          (i < 0 || i >= n ? ", which is out of range" : ", which is a site already"));
            return 1;
        }
        is_site[i] = 1;
    }
    std::vector<std::vector<int>> entries((size_t)n);
    for (int s = 0; s < n_sites; ++s) {
        const int kind = h_kind[s];
        if (kind != AMM_VSITE_AVERAGE2 && kind != AMM_VSITE_AVERAGE3 && kind != AMM_VSITE_OUT_OF_PLANE) {
            amm_set_error("amm_vsite_define: site " + std::to_string(s) + " has an unknown kind " + std::to_string(kind));
            return 1;
        }
        const int np = kind == AMM_VSITE_AVERAGE2 ? 2 : 3;
        for (int r = 0; r < 3; ++r) {
            const int p = h_parents[3 * s + r];
            if (r >= np) {
                if (p != -1) {
                    amm_set_error("amm_vsite_define: site " + std::to_string(s) + " of two parents must pad its third with -1");
                    return 1;
                }
                continue;
            }
            if (p < 0 || p >= n) {
                amm_set_error("amm_vsite_define: parent " + std::to_string(p) + " of site " + std::to_string(s) + " is out of range");
                return 1;
            }
            if (is_site[p]) {
                amm_set_error("amm_vsite_define: parent " + std::to_string(p) + " of site " + std::to_string(s) + " is a site itself");
                return 1;
            }
            for (int r2 = 0; r2 < r; ++r2)
                if (h_parents[3 * s + r2] == p) {
                    amm_set_error("amm_vsite_define: site " + std::to_string(s) + " names parent " + std::to_string(p) + " twice");
                    return 1;
                }
            if (!std::isfinite(h_weights[3 * s + r])) {
                amm_set_error("amm_vsite_define: site " + std::to_string(s) + " has a weight that is not finite");
                return 1;
            }
            entries[p].push_back(4 * s + r);          // (s ascends: every parent's entries are sorted by site)
        }
    }
    AMM_HIP(hipStreamSynchronize(ctx->stream));          // a launch that reads the old tables may still be queued
    amm_vsite_free(ctx);
    if (n_sites == 0) return 0;
    std::vector<int> owner, optr(1, 0), oent;
    for (int i = 0; i < n; ++i) {
        if (entries[i].empty()) continue;
        owner.push_back(i);
        oent.insert(oent.end(), entries[i].begin(), entries[i].end());
        optr.push_back((int)oent.size());
    }
    VsiteSet *vs = new VsiteSet();
    ctx->vsites = vs;            // (owned by the context from here on: a failed upload is freed with it)
    vs->n_sites = n_sites;
    vs->n_owners = (int)owner.size();
    auto up = [&](int **d, const int *h, size_t count) -> int {
        AMM_HIP(hipMalloc(d, sizeof(int) * count));
        AMM_HIP(hipMemcpy(*d, h, sizeof(int) * count, hipMemcpyHostToDevice));
        return 0;
    };
    if (up(&vs->d_site, h_site, (size_t)n_sites) || up(&vs->d_kind, h_kind, (size_t)n_sites) || up(&vs->d_parents, h_parents, 3 * (size_t)n_sites) ||
        up(&vs->d_owner, owner.data(), owner.size()) || up(&vs->d_optr, optr.data(), optr.size()) || up(&vs->d_oent, oent.data(), oent.size())) {
        amm_vsite_free(ctx);
        return 1;
    }
    if (hipMalloc(&vs->d_weights, sizeof(double) * 3 * (size_t)n_sites) != hipSuccess ||
        hipMemcpy(vs->d_weights, h_weights, sizeof(double) * 3 * (size_t)n_sites, hipMemcpyHostToDevice) != hipSuccess) {
        amm_vsite_free(ctx);
        amm_set_error("amm_vsite_define: the weights could not be uploaded");
        return 1;
    }
    return 0;
}

int amm_vsite_place_impl(amm_ctx *ctx, double *d_x) {
    VsiteSet *vs = ctx->vsites;
    if (!vs) return 0;
    VsiteArgs A;
    vsite_args(vs, A);
    hipLaunchKernelGGL(k_vsite_place, dim3((vs->n_sites + 255) / 256), dim3(256), 0, ctx->stream, A, d_x);
    AMM_HIP(hipGetLastError());
    vs->n_place++;
    vs->n_launches++;
    return 0;
}

int amm_vsite_spread_impl(amm_ctx *ctx, const double *d_x, double *d_f) {
    VsiteSet *vs = ctx->vsites;
    if (!vs) return 0;
    VsiteArgs A;
    vsite_args(vs, A);
    hipLaunchKernelGGL(k_vsite_spread, dim3((vs->n_owners + 255) / 256), dim3(256), 0, ctx->stream, A, d_x, d_f);
    AMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vsite_zero, dim3((vs->n_sites + 255) / 256), dim3(256), 0, ctx->stream, A, d_f);
    AMM_HIP(hipGetLastError());
    vs->n_spread++;
    vs->n_launches += 2;
    return 0;
}

int amm_vsite_stats_impl(amm_ctx *ctx, int64_t out[4]) {
    const VsiteSet *vs = ctx->vsites;
    out[0] = vs ? vs->n_place : 0;
    out[1] = vs ? vs->n_spread : 0;
    out[2] = vs ? vs->n_launches : 0;
    out[3] = vs ? vs->n_sites : 0;
    return 0;
}
