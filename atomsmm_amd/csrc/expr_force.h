// atomsmm_amd/csrc/expr_force.h -- what the force families that evaluate a user-written energy text share, stated once: the
// compiled program as host and device hold it and how it is filled, uploaded and given new globals; the variable table of the
// families whose text reads geometric variables (compound.hip, hbond.hip, manyparticle.hip) and its validation; the CSR builders
// of the parked-force gathers and of the exclusion lists; the half-box check of a cutoff; and, for the kernels, the staging of
// program and table into LDS and the search of a sorted exclusion row.  pair_expr_vm.h has the interpreter, compound_geom.h the
// geometry of a variable and the turns that differentiate a text by its variables, device_utils.h the block reduction of the
// energy and the write of a force row.  DESIGN.md 3 (`The kit of the text forces`) says what a new family takes from here.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>

#include "amm_ctx.h"

#define AMM_PEXPR_MAXCODE 256
#define AMM_PEXPR_MAXCONST 48
#define AMM_PEXPR_MAXGLOBAL 48

// the compiled text as the device holds it: staged into LDS once per block
struct PairExprProg {
    int ncode, nconst, nglobal, pad_;
    int code[AMM_PEXPR_MAXCODE];            // opcode | arg << 8
    double consts[AMM_PEXPR_MAXCONST];
    double globals[AMM_PEXPR_MAXGLOBAL];
};

// ---- host: the program of one force (the counts were checked by amm_expr_program_validate)
struct ExprProgram {
    PairExprProg h;
    PairExprProg *d = nullptr;
    void fill(const int32_t *code, int ncode, const double *consts, int nconst, const double *globals, int nglobal) {
        std::memset(&h, 0, sizeof(h));
        h.ncode = ncode;
        h.nconst = nconst;
        h.nglobal = nglobal;
        std::copy(code, code + ncode, h.code);
        std::copy(consts, consts + nconst, h.consts);
        std::copy(globals, globals + nglobal, h.globals);
    }
    int upload(amm_ctx *ctx, bool globals_only) {
        AMM_HIP(hipStreamSynchronize(ctx->stream));     // ordered after any kernel already queued on the stream that reads the old program
        if (!d) AMM_HIP(hipMalloc(&d, sizeof(PairExprProg)));
        if (globals_only) AMM_HIP(hipMemcpy(d->globals, h.globals, sizeof(h.globals), hipMemcpyHostToDevice));
        else AMM_HIP(hipMemcpy(d, &h, sizeof(PairExprProg), hipMemcpyHostToDevice));
        return 0;
    }
    int set_globals(amm_ctx *ctx, const char *who, const double *globals, int nglobal) {      // who: the entry point, for the message
        if (nglobal != h.nglobal || (nglobal > 0 && !globals)) {
            amm_set_error(std::string(who) + ": the program reads " + std::to_string(h.nglobal) + " globals, " + std::to_string(nglobal) + " given");
            return 1;
        }
        std::copy(globals, globals + nglobal, h.globals);
        return upload(ctx, true);
    }
    void release() {
        if (d) (void)hipFree(d);
        d = nullptr;
    }
};

// ---- the variable table as the device holds it
struct VarTable {
    int kind[AMM_COMPOUND_MAX_VARS];    // AMM_CVAR_*
    int4 slot[AMM_COMPOUND_MAX_VARS];   // positions within the bond (pair, set) of the variable's roles (0 behind its arity)
};

__host__ __device__ inline int cvar_arity(int kind) { return kind <= AMM_CVAR_Z ? 1 : kind - 1; }      // 1, 1, 1, 2, 3, 4

// Checks var_kinds (min_kind .. AMM_CVAR_DIHEDRAL) and the slots each variable reads (0 .. n_slots - 1), fills `tab` and marks in
// used[0 .. n_slots) the slots the text names (used may be null).  The family words its own refusals: "variable K has " +
// kind_before + kind + kind_after, and "variable K names slot S " + slot_tail.
inline int var_table_fill(const char *who, const int32_t *var_kinds, const int32_t *var_slots, int n_vars, int n_slots, int min_kind,
                          const char *kind_before, const char *kind_after, const std::string &slot_tail, VarTable &tab, bool *used) {
    auto fail = [who](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what);
        return 1;
    };
    std::memset(&tab, 0, sizeof(tab));
    for (int k = 0; k < n_vars; ++k) {
        const int kind = var_kinds[k];
        if (kind < min_kind || kind > AMM_CVAR_DIHEDRAL) return fail("variable " + std::to_string(k) + " has " + kind_before + std::to_string(kind) + kind_after);
        tab.kind[k] = kind;
        int s[4] = {0, 0, 0, 0};
        for (int r = 0; r < cvar_arity(kind); ++r) {
            s[r] = var_slots[4 * k + r];
            if (s[r] < 0 || s[r] >= n_slots) return fail("variable " + std::to_string(k) + " names slot " + std::to_string(s[r]) + " " + slot_tail);
            if (used) used[s[r]] = true;
        }
        tab.slot[k] = make_int4(s[0], s[1], s[2], s[3]);
    }
    return 0;
}

// ---- CSR builders
// Rows <- records visited in a given order: each(visit) calls visit(row, record) for every record, and is run twice (count, then
// fill).  The records of a row come out in the order of the visits -- which is the order a gather adds them in.
template <class Each>
inline void csr_of_records(int n_rows, Each &&each, std::vector<int> &ptr, std::vector<int> &src) {
    ptr.assign(n_rows + 1, 0);
    each([&](int row, int) { ptr[row + 1]++; });
    for (int i = 0; i < n_rows; ++i) ptr[i + 1] += ptr[i];
    src.resize(ptr[n_rows]);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    each([&](int row, int rec) { src[fill[row]++] = rec; });
}

// (row, column) pairs in any order, some maybe twice -> sorted and unique, and the CSR of a row's columns, ascending
inline void csr_of_pairs(int n_rows, std::vector<std::pair<int, int>> &pairs, std::vector<int> &ptr, std::vector<int> &col) {
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    ptr.assign(n_rows + 1, 0);
    col.resize(pairs.size());
    for (const auto &e : pairs) ptr[e.first + 1]++;
    for (int i = 0; i < n_rows; ++i) ptr[i + 1] += ptr[i];
    for (size_t e = 0; e < pairs.size(); ++e) col[e] = pairs[e].second;
}

// a periodic cutoff needs the minimum image to be the only image inside it (the box may have changed since creation: a barostat)
inline bool amm_cutoff_fits_box(amm_ctx *ctx, double rc, const char *who) {
    const double shortest = std::min(ctx->box.L[0], std::min(ctx->box.L[1], ctx->box.L[2]));
    if (rc > 0.5 * shortest) {
        amm_set_error(std::string(who) + ": the cutoff " + std::to_string(rc) + " exceeds half the shortest box edge (" + std::to_string(shortest) + ")");
        return false;
    }
    return true;
}

#ifdef __HIPCC__
// ---- device: every lane of the block takes part; the caller declares the arrays and has the barrier
__device__ __forceinline__ void pexpr_stage(const PairExprProg *__restrict__ prog, int *s_code, double *s_consts, double *s_globals) {
    const int ncode = prog->ncode;
    for (int k = threadIdx.x; k < ncode; k += blockDim.x) s_code[k] = prog->code[k];
    for (int k = threadIdx.x; k < prog->nconst; k += blockDim.x) s_consts[k] = prog->consts[k];
    for (int k = threadIdx.x; k < prog->nglobal; k += blockDim.x) s_globals[k] = prog->globals[k];
}

__device__ __forceinline__ void var_table_stage(const VarTable *__restrict__ tab, int *s_kind, int4 *s_slot) {
    if (threadIdx.x < AMM_COMPOUND_MAX_VARS) {
        s_kind[threadIdx.x] = tab->kind[threadIdx.x];
        s_slot[threadIdx.x] = tab->slot[threadIdx.x];
    }
}

// is x in the sorted list[lo .. hi)?
__device__ __forceinline__ bool sorted_contains(const int *__restrict__ list, int lo, int hi, int x) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && list[lo] == x;
}
#endif
