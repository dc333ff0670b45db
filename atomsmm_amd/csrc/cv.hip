// atomsmm_amd/csrc/cv.hip -- CustomCVForce with ANY energy text over several collective variables (AMM_FORCE_CV): a composite force
// that owns K inner force objects (bond-list sets or term-expression forces; each one's potential energy is collective variable k)
// and one compiled outer program f(cv_1 .. cv_K; globals) (atomsmm_amd/expr.py: compile_cv).
//
// Takes over what OpenMM does for this class: the inner forces are evaluated (OpenMM: in an inner Context), the outer expression
// and its partial derivatives are evaluated at their energies (Lepton differentiates the text; here the interpreter of
// pair_expr_vm.h carries one derivative along per lane), and the atoms get  -sum_k df/dcv_k grad cv_k.
//
//   1. K inner evaluations through amm_force_eval_dispatch, inner k writing -grad cv_k into row block k of the object's own
//      [K][n][3] scratch and adding cv_k into d_cv[k] (cleared first).
//   2. ONE launch, k_cv_apply.  Every block stages the program, the K values and the P derivative parameters in LDS; its first
//      32 lanes run pexpr_run<CvLeaves>, lane l seeding variable l (0 .. K-1: the collective variables, K .. K+P-1: the parameters
//      the force asked derivatives for, compiled as variables so that they can be seeded) and leaving df/dvar_l in coef[l]; after a
//      barrier the block combines its slice of the flat 3n doubles, out[i] (+)= sum_k coef[k] * fcv[k][i], k in the order 0 .. K-1.
//      Block 0 adds f to the energy and stores coef and the values for the read-backs (amm_cv_values, amm_cv_energy_derivative).
//      The outer program is at most 256 words on at most 32 lanes: repeating it in every block costs less than a launch of its own
//      (and the dependent launch's wait for it); DESIGN.md 3.CV has the figures.
//
// No atomics: a row of the output has one producer, the sum over k has a fixed order and fp contraction is off -- the same bits
// run to run, and with the outer text `cv1` the numbers of the inner force itself.
#include <algorithm>
#include <cstring>

#include "amm_ctx.h"
#include "term_expr_vm.h"

#define AMM_CV_LANES 32                 // lanes of the outer pass = AMM_CV_MAX_CVS + AMM_CV_MAX_DERIVS: one per variable
#define AMM_CV_BLOCK 256
#define AMM_CV_PER_LANE 4               // doubles of the flat force array a lane combines

struct CvForce {
    int n_cv = 0, n_deriv = 0;
    int inner[AMM_CV_MAX_CVS];
    ExprProgram prog;                   // the outer program: layout and limits of a pair expression's
    double h_vars[AMM_CV_MAX_DERIVS];   // current values of the derivative parameters
    double *d_vars = nullptr;           // [P] the same on the device
    double *d_cv = nullptr;             // [K] the inner energies of the evaluation in flight
    double *d_fcv = nullptr;            // [K][n][3] -grad cv_k
    double *d_coef = nullptr;           // [K + P] df/dvar of the last evaluation, then [K] its values (block 0 stores them)
};

// The leaves of the outer text: variable k is TERM_VAR k, read from the block's staged values; the seed is this lane's one-hot.
struct CvLeaves {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_CV_LANES;
    const double *vars;
    int lane;
    __device__ __forceinline__ double var(int k) const { return vars[k]; }
    __device__ __forceinline__ double seed(int k) const { return k == lane ? 1.0 : 0.0; }
    __device__ __forceinline__ double param(int) const { return 0.0; }       // (no per-term parameters: the validator refuses the word)
};

struct CvArgs {
    int K, P, accumulate;
    long n3;                    // doubles of a force buffer: 3 n
    const double *cv;           // [K]
    const double *vars;         // [P]
    const double *fcv;          // [K][n3]
    double *out;                // [n3], or nullptr: the outer pass only (amm_cv_energy_derivative)
    double *energy;             // added to, or nullptr
    double *coef;               // [K + P] then [K]
    double *dout;               // [P] added to, or nullptr
};

__global__ void __launch_bounds__(AMM_CV_BLOCK) k_cv_apply(CvArgs A, const PairExprProg *__restrict__ prog) {
#pragma clang fp contract(off)
    __shared__ int s_code[AMM_PEXPR_MAXCODE];
    __shared__ double s_consts[AMM_PEXPR_MAXCONST];
    __shared__ double s_globals[AMM_PEXPR_MAXGLOBAL];
    __shared__ double s_var[AMM_CV_LANES];
    __shared__ double s_coef[AMM_CV_LANES];
    __shared__ double s_energy;
    __shared__ double2 s_stack[(AMM_PEXPR_STACK - 1) * AMM_CV_LANES];
    const int ncode = prog->ncode, nv = A.K + A.P;
    pexpr_stage(prog, s_code, s_consts, s_globals);
    if (threadIdx.x < AMM_CV_LANES) s_var[threadIdx.x] = threadIdx.x < A.K ? A.cv[threadIdx.x] : (threadIdx.x < nv ? A.vars[threadIdx.x - A.K] : 0.0);
    __syncthreads();
    if (threadIdx.x < nv) {             // (nv <= 32: half of the first wavefront, one lane per partial derivative)
        CvLeaves L;
        L.vars = s_var;
        L.lane = threadIdx.x;
        double e, de;
        pexpr_run(s_code, ncode, s_consts, s_globals, L, s_stack + threadIdx.x, e, de);
        s_coef[threadIdx.x] = de;
        if (threadIdx.x == 0) s_energy = e;
    }
    __syncthreads();
    if (A.out) {
        const long base = (long)blockIdx.x * (AMM_CV_BLOCK * AMM_CV_PER_LANE) + threadIdx.x;
#pragma unroll
        for (int u = 0; u < AMM_CV_PER_LANE; ++u) {
            const long i = base + (long)u * AMM_CV_BLOCK;
            if (i < A.n3) {
                double s = s_coef[0] * A.fcv[i];
                for (int k = 1; k < A.K; ++k) s += s_coef[k] * A.fcv[(long)k * A.n3 + i];
                A.out[i] = A.accumulate ? A.out[i] + s : s;
            }
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < nv) A.coef[threadIdx.x] = s_coef[threadIdx.x];
        if (threadIdx.x < A.K) A.coef[nv + threadIdx.x] = s_var[threadIdx.x];
        if (A.dout && threadIdx.x < A.P) A.dout[threadIdx.x] += s_coef[A.K + threadIdx.x];
        if (A.energy && threadIdx.x == 0) *A.energy += s_energy;
    }
}

// every inner id still names a bond-list set, a term-expression force or a compound-bond force (who: the entry point, for the message)
static int cv_check_inner(amm_ctx *ctx, const int32_t *inner, int n_cv, const char *who) {
    for (int k = 0; k < n_cv; ++k) {
        const int id = inner[k];
        if (id < 0 || id >= (int)ctx->forces.size()) {
            amm_set_error(std::string(who) + ": inner force " + std::to_string(k) + " has id " + std::to_string(id) + ", which is no force of this context");
            return 1;
        }
        const int type = ctx->forces[id].type;
        if (type != AMM_FORCE_BONDED && type != AMM_FORCE_TERM_EXPR && type != AMM_FORCE_COMPOUND && type != AMM_FORCE_RMSD) {
            amm_set_error(std::string(who) + ": inner force " + std::to_string(k) + " (id " + std::to_string(id) + ") is " + amm_family(type).noun +
                          " (" + amm_family(type).tag + "): a collective variable is the energy of a bond-list set, of a term-expression force, of a compound-bond force or of an RMSD force");
            return 1;
        }
    }
    return 0;
}

// the K inner evaluations: -grad cv_k into block k of d_fcv, cv_k into d_cv[k]
static int cv_eval_inner(amm_ctx *ctx, CvForce *cv, const double *d_pos, const char *who) {
    if (cv_check_inner(ctx, cv->inner, cv->n_cv, who)) return 1;        // (an inner id released since creation: before anything launches)
    const size_t n3 = 3 * (size_t)ctx->n;
    AMM_HIP(hipMemsetAsync(cv->d_cv, 0, sizeof(double) * cv->n_cv, ctx->stream));
    for (int k = 0; k < cv->n_cv; ++k)
        if (amm_force_eval_dispatch(ctx, cv->inner[k], d_pos, cv->d_fcv + (size_t)k * n3, 0, cv->d_cv + k)) return 1;
    return 0;
}

static int cv_apply(amm_ctx *ctx, CvForce *cv, double *d_force, int accumulate, double *d_energy, double *d_dout) {
    CvArgs A;
    A.K = cv->n_cv;
    A.P = cv->n_deriv;
    A.accumulate = accumulate;
    A.n3 = 3 * (long)ctx->n;
    A.cv = cv->d_cv;
    A.vars = cv->d_vars;
    A.fcv = cv->d_fcv;
    A.out = d_force;
    A.energy = d_energy;
    A.coef = cv->d_coef;
    A.dout = d_dout;
    const long per_block = AMM_CV_BLOCK * AMM_CV_PER_LANE;
    const int blocks = d_force ? (int)std::max<long>(1, (A.n3 + per_block - 1) / per_block) : 1;
    hipLaunchKernelGGL(k_cv_apply, dim3(blocks), dim3(AMM_CV_BLOCK), 0, ctx->stream, A, cv->prog.d);
    AMM_HIP(hipGetLastError());
    return 0;
}

int amm_cv_eval_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    if (cv_eval_inner(ctx, cv, d_pos, "evaluation of a collective-variable force (AMM_FORCE_CV)")) return 1;
    return cv_apply(ctx, cv, d_force, accumulate, d_energy, nullptr);
}

int amm_cv_create_impl(amm_ctx *ctx, const int32_t *inner_ids, int n_cv, int n_deriv, const int32_t *code, int ncode, const double *consts,
                       int nconst, const double *globals, int nglobal, CvForce **out) {
    auto fail = [](const std::string &what) {
        amm_set_error("amm_cv_create: " + what);
        return 1;
    };
    if (n_cv < 1 || n_cv > AMM_CV_MAX_CVS) return fail(std::to_string(n_cv) + " collective variables (1 .. " + std::to_string(AMM_CV_MAX_CVS) + ")");
    if (n_deriv < 0 || n_deriv > AMM_CV_MAX_DERIVS) return fail(std::to_string(n_deriv) + " derivative parameters (limit " + std::to_string(AMM_CV_MAX_DERIVS) + ")");
    if (ctx->world > 1) return fail("a collective-variable force (AMM_FORCE_CV) runs on a single rank");
    if (cv_check_inner(ctx, inner_ids, n_cv, "amm_cv_create")) return 1;
    if (amm_expr_program_validate("amm_cv_create", code, ncode, nconst, nglobal, n_cv + n_deriv, 0)) return 1;
    AMM_HIP(hipSetDevice(ctx->device));
    CvForce *cv = new CvForce();
    cv->n_cv = n_cv;
    cv->n_deriv = n_deriv;
    std::copy(inner_ids, inner_ids + n_cv, cv->inner);
    std::memset(cv->h_vars, 0, sizeof(cv->h_vars));
    cv->prog.fill(code, ncode, consts, nconst, globals, nglobal);
    const size_t n3 = 3 * (size_t)ctx->n;
    auto alloc = [&]() {
        AMM_HIP(hipMalloc(&cv->d_vars, sizeof(double) * AMM_CV_MAX_DERIVS));
        AMM_HIP(hipMalloc(&cv->d_cv, sizeof(double) * AMM_CV_MAX_CVS));
        AMM_HIP(hipMalloc(&cv->d_coef, sizeof(double) * (AMM_CV_MAX_CVS + AMM_CV_MAX_DERIVS + AMM_CV_MAX_CVS)));
        AMM_HIP(hipMalloc(&cv->d_fcv, sizeof(double) * n3 * n_cv));
        AMM_HIP(hipMemset(cv->d_vars, 0, sizeof(double) * AMM_CV_MAX_DERIVS));
        AMM_HIP(hipMemset(cv->d_cv, 0, sizeof(double) * AMM_CV_MAX_CVS));
        AMM_HIP(hipMemset(cv->d_coef, 0, sizeof(double) * (AMM_CV_MAX_CVS + AMM_CV_MAX_DERIVS + AMM_CV_MAX_CVS)));
        return cv->prog.upload(ctx, false);
    };
    if (alloc()) {
        amm_cv_free(cv);
        return 1;
    }
    *out = cv;
    return 0;
}

int amm_cv_set_globals_impl(amm_ctx *ctx, CvForce *cv, const double *globals, int nglobal) {
    return cv->prog.set_globals(ctx, "amm_cv_set_globals", globals, nglobal);
}

int amm_cv_set_variables_impl(amm_ctx *ctx, CvForce *cv, const double *values, int n_deriv) {
    if (n_deriv != cv->n_deriv || (n_deriv > 0 && !values)) {
        amm_set_error("amm_cv_set_variables: the force has " + std::to_string(cv->n_deriv) + " derivative parameters, " + std::to_string(n_deriv) + " given");
        return 1;
    }
    if (!n_deriv) return 0;
    std::copy(values, values + n_deriv, cv->h_vars);
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    AMM_HIP(hipMemcpy(cv->d_vars, cv->h_vars, sizeof(double) * n_deriv, hipMemcpyHostToDevice));
    return 0;
}

// the one synchronising call: the inner energies at d_pos, copied out
int amm_cv_values_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *h_out) {
    if (cv_eval_inner(ctx, cv, d_pos, "amm_cv_values")) return 1;
    AMM_HIP(hipMemcpyAsync(h_out, cv->d_cv, sizeof(double) * cv->n_cv, hipMemcpyDeviceToHost, ctx->stream));
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// df/dp of the P derivative parameters at d_pos, ADDED to d_out[0 .. P) on the stream (no wait: amm_pair_energy_derivative's shape)
int amm_cv_energy_derivative_impl(amm_ctx *ctx, CvForce *cv, const double *d_pos, double *d_out) {
    if (cv_eval_inner(ctx, cv, d_pos, "amm_cv_energy_derivative")) return 1;
    return cv_apply(ctx, cv, nullptr, 0, nullptr, d_out);
}

void amm_cv_free(CvForce *cv) {
    if (!cv) return;
    for (void *p : {(void *)cv->prog.d, (void *)cv->d_vars, (void *)cv->d_cv, (void *)cv->d_fcv, (void *)cv->d_coef})
        if (p) (void)hipFree(p);
    delete cv;
}
