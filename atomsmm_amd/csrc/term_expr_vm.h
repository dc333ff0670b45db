// atomsmm_amd/csrc/term_expr_vm.h -- the term-expression side of the interpreter of pair_expr_vm.h: the energy text of a
// CustomBondForce / CustomAngleForce / CustomTorsionForce / CustomExternalForce that is none of the hand-written kinds, compiled by
// atomsmm_amd/expr.py (compile_term) and evaluated per term by k_term_expr (term_expr.hip).
//
// The op switch is pexpr_run's, instantiated with other leaves: X_TERM_VAR k pushes (var[k], seed[k]) -- the term's geometric
// variable with the derivative seed of this pass: (r, 1), (theta, 1), or x, y, z with one of (1,0,0), (0,1,0), (0,0,1) -- and
// X_TERM_P k pushes (param[k], 0).  The parameters stay in global memory, parameter-major: lane t reads p[k * n_terms + t] when the
// program asks for it, neighbouring lanes neighbouring doubles, and no register holds a parameter the text never reads.
#pragma once
#include "pair_expr_vm.h"

// host side of one such force (AMM_FORCE_TERM_EXPR)
struct TermExprForce {
    int kind = 0, periodic = 0;
    int n_terms = 0, n_params = 0, arity = 0;
    ExprProgram prog;               // the program: same layout and limits as a pair expression's
    int4 *d_atoms = nullptr;        // [n_terms] atoms of the term (-1 padded)
    double *d_params = nullptr;     // [n_params][n_terms]
    int *d_ref_ptr = nullptr;       // [n + 1] CSR per atom of its (term, role) records ...
    int *d_rec_src = nullptr;       // [n_terms * arity] ... each term * 4 + role, in term order
    double *d_tf = nullptr;         // [n_terms][4][3] parked forces of the terms' roles
    double *d_epart = nullptr;      // [blocks of k_term_expr] energy partial sums
    int n_blocks = 0;
};

// non-zero + message (prefixed with `who`) naming the limit that a program exceeds, or a word that is no op of its kind / leaves the
// stack or the locals.  term_vars < 0: a pair program (X_PAIR_* leaves); else a term program over that many variables and
// term_params parameters (X_TERM_* leaves); term_tables: ... that may also hold the table words (custom_gb.hip).
int amm_term_arity(int kind);     // atoms of a term of kind AMM_TERM_*: 2, 3, 4, 1 (term_expr.hip)
int amm_expr_program_validate(const char *who, const int32_t *code, int ncode, int nconst, int nglobal, int term_vars, int term_params,
                              bool term_tables = false);

#ifdef __HIPCC__
// NV: the kind's variables.  3: x, y, z and the seed of this pass, indexed by the word's argument.
template <int NV>
struct TermLeaves {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_PEXPR_STRIDE;
    double v[3], s[3];
    const double *p;                // the lane's column of the parameter array
    size_t stride;                  // n_terms
    __device__ __forceinline__ double var(int k) const { return v[k]; }
    __device__ __forceinline__ double seed(int k) const { return s[k]; }
    __device__ __forceinline__ double param(int k) const { return p[(size_t)k * stride]; }
};
// 1: r or theta, seed 1 -- no array, so nothing for the compiler to index (and to place in LDS or scratch)
template <>
struct TermLeaves<1> {
    static constexpr bool kPair = false;
    static constexpr int kStride = AMM_PEXPR_STRIDE;
    double v;
    const double *p;
    size_t stride;
    __device__ __forceinline__ double var(int) const { return v; }
    __device__ __forceinline__ double seed(int) const { return 1.0; }
    __device__ __forceinline__ double param(int k) const { return p[(size_t)k * stride]; }
};
#endif
