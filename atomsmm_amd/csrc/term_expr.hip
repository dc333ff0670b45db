// atomsmm_amd/csrc/term_expr.hip -- generic bond-list terms: a CustomBondForce / CustomAngleForce / CustomTorsionForce /
// CustomExternalForce whose energy text is none of the hand-written kinds of bonded_terms.h (AMM_FORCE_TERM_EXPR), evaluated by
// interpreting the compiled text per term (term_expr_vm.h: the interpreter of pair_expr_vm.h with other leaves).
//
// Takes over what OpenMM does for these four classes: per term, the energy expression in the term's geometric variable and its
// derivative (Lepton differentiates the text; here the interpreter carries the derivative along), times the gradient of the variable.
// The geometry is that of the hand-written kinds -- delta3 / cross3 / amm_min_image of bonded_terms.h, the angle gradient of
// AMM_ANGLE_HARMONIC with its 1 - c^2 floor, the dihedral convention and gradient of AMM_TORSION_PERIODIC -- so a text that restates
// one of them gives its numbers to rounding.  An external term reads raw coordinates and runs the program three times, seeded
// (1,0,0), (0,1,0), (0,0,1).
//
// Two launches, no atomics, the pattern of k_terms_eval / k_terms_gather (bonded.hip): k_term_expr evaluates one term per lane and
// parks the forces of its roles (twelve doubles per term); k_term_expr_gather, one lane per atom, adds the atom's (term, role)
// records in record order from a CSR built at creation, and writes every row (zeros for atoms in no term) when it does not
// accumulate.  The energy goes through a fixed-order block reduction into per-block partials (amm_reduce_add sums them in order).
// The energy instantiation computes the forces with the same operations as the force-only one: same bits.
//
// Layout: code, constants and globals are staged once per block in LDS and read back wave-uniformly; the top of each lane's stack is
// a register pair, the 15 slots below it the lane's column of an LDS strip (15 x 256 lanes x 16 B = 60 KiB per block, two blocks
// per CU -- k_pair_expr's budget); per-term parameters are read parameter-major from global memory when the program asks for one.
// DESIGN.md 3.TE has the resource figures and the measured cost.
#include <algorithm>
#include <cstring>

#include "amm_ctx.h"
#include "bonded_terms.h"
#include "device_utils.h"
#include "term_expr_vm.h"

struct TermArgs {
    int n_terms, periodic;
    const int4 *atoms;
    const double *params;
    const double *pos;
    double *tf;
    double *epart;
    Box box;
};

template <int KIND, bool EN>
__global__ void __launch_bounds__(256) k_term_expr(TermArgs A, const PairExprProg *__restrict__ prog) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_PEXPR_STRIDE];      // all but the top of every lane's stack
    const int ncode = prog->ncode;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    double e = 0.0;
    if (t < A.n_terms) {
        const int4 at = A.atoms[t];
        const PosPlain pos{A.pos};
        double2 *st = s_stack + threadIdx.x;
        double *out = A.tf + (size_t)t * 12;
        TermLeaves<KIND == AMM_TERM_EXTERNAL ? 3 : 1> L;
        L.p = A.params + t;
        L.stride = (size_t)A.n_terms;
        double de;
        if constexpr (KIND == AMM_TERM_BOND) {
            double d[3];
            delta3(pos, at.x, at.y, A.box, A.periodic, d);
            const double r = sqrt(dot3(d, d));
            L.v = r;
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, e, de);
            const double fr = -de / r;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double f = fr * d[x];
                out[x] = f;
                out[3 + x] = -f;
            }
        } else if constexpr (KIND == AMM_TERM_ANGLE) {
            double d1[3], d2[3];
            delta3(pos, at.x, at.y, A.box, A.periodic, d1);
            delta3(pos, at.z, at.y, A.box, A.periodic, d2);
            const double i1 = amm_rsqrt(dot3(d1, d1)), i2 = amm_rsqrt(dot3(d2, d2));
            double c = dot3(d1, d2) * i1 * i2;
            c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
            L.v = acos(c);
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, e, de);
            double s2 = 1.0 - c * c;
            if (s2 < 1e-24) s2 = 1e-24;
            const double g = de * amm_rsqrt(s2);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double u1 = d1[x] * i1, u2 = d2[x] * i2;      // unit vectors
                const double fi = g * (u2 - c * u1) * i1;
                const double fk = g * (u1 - c * u2) * i2;
                out[x] = fi;
                out[3 + x] = -(fi + fk);
                out[6 + x] = fk;
            }
        } else if constexpr (KIND == AMM_TERM_TORSION) {
            double F[3], G[3], H[3], Av[3], Bv[3], BA[3];
            delta3(pos, at.x, at.y, A.box, A.periodic, F);
            delta3(pos, at.y, at.z, A.box, A.periodic, G);
            delta3(pos, at.w, at.z, A.box, A.periodic, H);
            cross3(F, G, Av);
            cross3(H, G, Bv);
            cross3(Bv, Av, BA);
            const double Gn = sqrt(dot3(G, G));
            L.v = atan2(dot3(BA, G) / Gn, dot3(Av, Bv));
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, e, de);
            const double A2 = dot3(Av, Av), B2 = dot3(Bv, Bv), FG = dot3(F, G), HG = dot3(H, G);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double gi = -Gn / A2 * Av[x], gl = Gn / B2 * Bv[x];
                const double gj = Gn / A2 * Av[x] + FG / (A2 * Gn) * Av[x] - HG / (B2 * Gn) * Bv[x];
                const double gk = -Gn / B2 * Bv[x] - FG / (A2 * Gn) * Av[x] + HG / (B2 * Gn) * Bv[x];
                out[x] = -(de * gi);
                out[3 + x] = -(de * gj);
                out[6 + x] = -(de * gk);
                out[9 + x] = -(de * gl);
            }
        } else {        // AMM_TERM_EXTERNAL
            L.v[0] = pos.get(at.x, 0);
            L.v[1] = pos.get(at.x, 1);
            L.v[2] = pos.get(at.x, 2);
            L.s[0] = 1.0;
            L.s[1] = L.s[2] = 0.0;
            double ey, ez, dy, dz;
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, e, de);
            L.s[0] = 0.0;
            L.s[1] = 1.0;
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, ey, dy);
            L.s[1] = 0.0;
            L.s[2] = 1.0;
            pexpr_run(s_code, ncode, s_consts, s_globals, L, st, ez, dz);
            out[0] = -de;
            out[1] = -dy;
            out[2] = -dz;
        }
    }
    if (EN) block_energy_store_256(e, A.epart);
}

// one lane per atom: its records, in record order (k_terms_gather's loop: four records in flight)
__global__ void __launch_bounds__(256) k_term_expr_gather(int n, const int *__restrict__ ref_ptr, const int *__restrict__ rec_src,
                                                          const double *__restrict__ tf, double *__restrict__ force, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double f[3] = {0.0, 0.0, 0.0};
    const int rb = ref_ptr[i], re = ref_ptr[i + 1];
    for (int r0 = rb; r0 < re; r0 += 4) {
        int src[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) src[u] = r0 + u < re ? rec_src[r0 + u] : -1;
        double g[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int x = 0; x < 3; ++x) g[u][x] = src[u] >= 0 ? tf[(size_t)src[u] * 3 + x] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (src[u] >= 0) {
#pragma unroll
                for (int x = 0; x < 3; ++x) f[x] += g[u][x];
            }
    }
    if (accumulate) {        // (not store_force_row of device_utils.h: this gather keeps the parent's instructions, profiles/expr_kit_cost.txt)
        force[3 * i] += f[0]; force[3 * i + 1] += f[1]; force[3 * i + 2] += f[2];
    } else {
        force[3 * i] = f[0]; force[3 * i + 1] = f[1]; force[3 * i + 2] = f[2];
    }
}

template <int KIND>
static void launch_terms(amm_ctx *ctx, TermExprForce *tf, const TermArgs &A, bool en) {
    if (en) hipLaunchKernelGGL((k_term_expr<KIND, true>), dim3(tf->n_blocks), dim3(256), 0, ctx->stream, A, tf->prog.d);
    else hipLaunchKernelGGL((k_term_expr<KIND, false>), dim3(tf->n_blocks), dim3(256), 0, ctx->stream, A, tf->prog.d);
}

int amm_term_expr_eval_impl(amm_ctx *ctx, TermExprForce *tf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    const int n = ctx->n;
    if (tf->n_terms > 0) {
        TermArgs A;
        A.n_terms = tf->n_terms;
        A.periodic = tf->periodic;
        A.atoms = tf->d_atoms;
        A.params = tf->d_params;
        A.pos = d_pos;
        A.tf = tf->d_tf;
        A.epart = tf->d_epart;
        A.box = ctx->box;
        const bool en = d_energy != nullptr;
        switch (tf->kind) {
        case AMM_TERM_BOND: launch_terms<AMM_TERM_BOND>(ctx, tf, A, en); break;
        case AMM_TERM_ANGLE: launch_terms<AMM_TERM_ANGLE>(ctx, tf, A, en); break;
        case AMM_TERM_TORSION: launch_terms<AMM_TERM_TORSION>(ctx, tf, A, en); break;
        default: launch_terms<AMM_TERM_EXTERNAL>(ctx, tf, A, en); break;
        }
        AMM_HIP(hipGetLastError());
    }
    // (a force without terms still writes its rows: it may be the first member of its group)
    hipLaunchKernelGGL(k_term_expr_gather, dim3(std::max(1, (n + 255) / 256)), dim3(256), 0, ctx->stream, n, tf->d_ref_ptr, tf->d_rec_src,
                       tf->d_tf, d_force, accumulate);
    AMM_HIP(hipGetLastError());
    if (d_energy && tf->n_terms > 0) return amm_reduce_add(ctx, tf->d_epart, tf->n_blocks, 1.0, d_energy);
    return 0;
}

// ---- host: device arrays, uploads ----
static const int kTermArity[4] = {2, 3, 4, 1};
int amm_term_arity(int kind) { return kTermArity[kind]; }

// h_idx: n_terms x 4 (checked by the caller); h_params: [n_params][n_terms]
int amm_term_expr_build(amm_ctx *ctx, TermExprForce *tf, const int32_t *h_idx, const double *h_params) {
    const int n = ctx->n, nt = tf->n_terms, ar = kTermArity[tf->kind];
    tf->arity = ar;
    tf->n_blocks = std::max(1, (nt + 255) / 256);
    std::vector<int4> atoms(nt);
    for (int t = 0; t < nt; ++t) {
        const int32_t *ix = h_idx + (size_t)t * 4;
        atoms[t] = make_int4(ix[0], ar > 1 ? ix[1] : -1, ar > 2 ? ix[2] : -1, ar > 3 ? ix[3] : -1);
    }
    std::vector<int> ptr, src;
    csr_of_records(n, [&](auto &&visit) {           // term order, role order: the records of an atom come out in that order
        for (int t = 0; t < nt; ++t)
            for (int r = 0; r < ar; ++r) visit(h_idx[(size_t)t * 4 + r], t * 4 + r);
    }, ptr, src);
    AMM_HIP(hipMalloc(&tf->d_atoms, sizeof(int4) * std::max(nt, 1)));
    AMM_HIP(hipMalloc(&tf->d_params, sizeof(double) * std::max<size_t>((size_t)nt * tf->n_params, 1)));
    AMM_HIP(hipMalloc(&tf->d_ref_ptr, sizeof(int) * (n + 1)));
    AMM_HIP(hipMalloc(&tf->d_rec_src, sizeof(int) * std::max<size_t>(src.size(), 1)));
    AMM_HIP(hipMalloc(&tf->d_tf, sizeof(double) * 12 * std::max(nt, 1)));
    AMM_HIP(hipMalloc(&tf->d_epart, sizeof(double) * tf->n_blocks));
    AMM_HIP(hipMemset(tf->d_tf, 0, sizeof(double) * 12 * std::max(nt, 1)));
    if (nt) AMM_HIP(hipMemcpy(tf->d_atoms, atoms.data(), sizeof(int4) * nt, hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(tf->d_ref_ptr, ptr.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice));
    if (!src.empty()) AMM_HIP(hipMemcpy(tf->d_rec_src, src.data(), sizeof(int) * src.size(), hipMemcpyHostToDevice));
    if (amm_term_expr_upload_params(ctx, tf, h_params)) return 1;
    return tf->prog.upload(ctx, false);
}

int amm_term_expr_upload_params(amm_ctx *ctx, TermExprForce *tf, const double *h_params) {
    const size_t count = (size_t)tf->n_terms * tf->n_params;
    if (!count) return 0;
    AMM_HIP(hipStreamSynchronize(ctx->stream));     // ordered after any kernel already queued on the stream that reads the old values
    AMM_HIP(hipMemcpy(tf->d_params, h_params, sizeof(double) * count, hipMemcpyHostToDevice));
    return 0;
}

void amm_term_expr_free(TermExprForce *tf) {
    if (!tf) return;
    for (void *p : {(void *)tf->prog.d, (void *)tf->d_atoms, (void *)tf->d_params, (void *)tf->d_ref_ptr, (void *)tf->d_rec_src, (void *)tf->d_tf,
                    (void *)tf->d_epart})
        if (p) (void)hipFree(p);
    delete tf;
}
