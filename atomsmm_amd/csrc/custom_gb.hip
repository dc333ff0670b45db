// atomsmm_amd/csrc/custom_gb.hip -- CustomGBForce: a generalized-Born model written as text (computed per-particle values plus energy
// terms), for free-space systems (gfx950, fp64, wave64).  Type AMM_FORCE_CUSTOM_GB.  DESIGN.md 3.CG.
//
// The definition (include/atomsmm_hip.h: amm_custom_gb_create).  A pair (i, j), i != j, takes part when there is no cutoff or
// r^2 < rc^2; a text of type AMM_CGB_PAIR also wants (i, j) not excluded.
//   value 0, of a pair type:   V0_i = sum_j f(r; parameters of i, parameters of j) over the ordered pairs that take part
//   value k, single particle:  Vk_i = f(parameters of i, V0_i .. V(k-1)_i)
//   energy:  sum_i f(parameters of i, values of i)  +  sum_{i<j taking part} f(r; parameters and values of i and of j)
// and the force is the full chain rule: d/dr of the pair terms at fixed values, plus sum_i G0_i dV0_i/dx with G_i = dE/d(values of i)
// carried back through the single-particle values.
//
// Every text is a program of the interpreter of pair_expr_vm.h (pexpr_run), compiled by atomsmm_amd/expr.py (compile_custom_gb) over
// the leaves of CgbLeaves: variable 0 is r, 1 + k value k of atom 1 (or of the atom itself), 5 + k value k of atom 2; parameter k
// belongs to atom 1 (the atom itself), 8 + k to atom 2.  One run gives the text and its derivative along ONE of the variables -- the
// seed -- so a text is run once per variable it has to be differentiated in.
//
// Decomposition: that of gb.hip -- a block of 256 threads owns 256 >> lpr_shift rows, a row is summed by 1 .. 64 consecutive lanes that
// meet in a __shfl_xor butterfly, the j atoms come through LDS in tiles of 256, every pair is evaluated from both sides, no atomics,
// a fixed order of summation.  Up to four launches, each needing the completed sums of the one before:
//   1. k_cgb_value  (value 0 of a pair type only): tile (x, y, z, parameters).  Row i sums the value-0 program.
//   2. k_cgb_atom   one lane per atom: the single-particle value programs in order; stores Vk_i and dVm_i/dVk_i for every (m, k) the
//                   program of m reads (one seeded run each; zero for the others).
//   3. k_cgb_energy tile (x, y, z, parameters, values).  Per pair and pair term one run seeded in r and one per value of the ROW atom
//                   the term reads (a pair term is symmetric under 1 <-> 2: the neighbour's row collects its own side).  Row i sums its
//                   energy (half), the direct force and dE/dVk_i; the finish adds the single-particle terms, carries dE/dV back through
//                   the Jacobian to G0_i and parks the row's force (or stores it, when value 0 does not depend on the positions).
//   4. k_cgb_chain  (value 0 of a pair type only): tile (x, y, z, parameters, G0).  Row i gathers G0_i df(r; p_i, p_j)/dr and
//                   G0_j df(r; p_j, p_i)/dr -- two runs of the value-0 program with the roles swapped -- adds the parked row and
//                   stores once, honouring `accumulate`.
// A pair that does not take part is evaluated at r = 1 and discarded by a select: it contributes exact zeros.
//
// LDS, all of it in the dynamic region: the interpreter's stack strip (60 KiB per block), the tile (3 + parameters + values doubles per
// atom, at most 16: 32 KiB), and the constants, globals and code of the programs the pass runs.  The row atom's parameters and values
// are read from global memory when a program asks for them (every lane of a row reads the same double).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "amm_ctx.h"
#include "term_expr_vm.h"

#define AMM_CGB_TILE 256
#define AMM_CGB_BLOCK 256
#define AMM_CGB_MAX_PROGS (AMM_CGB_MAX_VALUES + AMM_CGB_MAX_TERMS)
#define AMM_CGB_VAR_V1 1            // variable 1 + k: value k of atom 1
#define AMM_CGB_VAR_V2 5            // variable 5 + k: value k of atom 2
#define AMM_CGB_NVARS 9
#define AMM_CGB_P2 8                // parameter 8 + k: parameter k of atom 2
#define AMM_CGB_NPARAMS 16
#define AMM_CGB_STRIP_BYTES ((AMM_PEXPR_STACK - 1) * AMM_PEXPR_STRIDE * 16)

// one program within the force's concatenated code and constants
struct CgbProg {
    int code_off, ncode, const_off, nconst;
    int type;                       // AMM_CGB_SINGLE / AMM_CGB_PAIR / AMM_CGB_PAIR_NOEXCL
    int reads;                      // bit k: the text reads value k of atom 1 (of the atom itself)
    int pad_[2];
};

struct CustomGbForce {
    int n = 0, np = 0, nv = 0, ne = 0, nglobal = 0;
    bool v0_pair = false, any_excl = false, uses_tables = false;
    double rc2 = 0;
    CgbProg progs[AMM_CGB_MAX_PROGS];       // the values' programs, then the energy terms'
    std::vector<int> h_code;
    std::vector<double> h_consts;
    int *d_code = nullptr;
    double *d_consts = nullptr, *d_globals = nullptr;
    double *d_params = nullptr;             // [np][n]
    double *d_V = nullptr;                  // [nv][n]
    double *d_J = nullptr;                  // [4 m + k][n]: dVm/dVk
    double *d_G0 = nullptr;                 // [n]
    double *d_fdir = nullptr;               // [n][3] rows of pass 3, read by pass 4
    int *d_excl_ptr = nullptr, *d_excl_idx = nullptr;
    double *d_epart = nullptr;
    int n_epart = 0;
    PairExpr *tabx = nullptr;               // the tabulated functions (pair_expr.hip: amm_pair_expr_tables); its program is empty
    int64_t n_evals = 0;
};

struct CgbArgs {
    int n, lpr_shift, accumulate, np, nv, ne, v0_pair, nglobal;
    int c0, c1, k0, k1;             // the code words and constants this pass stages
    int nf;                         // doubles per atom of the tile
    int any_excl;
    const double *pos, *params;
    double *V, *J, *G0, *fdir, *force, *epart;
    const int *excl_ptr, *excl_idx, *code;
    const double *consts, *globals;
    const PairTableDesc *tabs;
    double rc2;
    CgbProg progs[AMM_CGB_MAX_PROGS];
};

// The leaves of these programs.  pa / pb: parameter k of atom 1 / 2 at pa[k * sa] (global memory, parameter-major: stride n; the
// tile: stride 256); va / vb the values likewise.  seeded: the variable whose derivative this run carries (-1: none).
struct CgbLeaves {
    static constexpr bool kPair = false;
    static constexpr bool kTables = true;
    static constexpr int kStride = AMM_PEXPR_STRIDE;
    double r;
    int seeded;
    const double *pa;
    int sa;
    const double *pb;
    int sb;
    const double *va;
    int sva;
    const double *vb;
    int svb;
    const PairTableDesc *tabs;
    __device__ __forceinline__ double var(int k) const {
        return k == 0 ? r : (k < AMM_CGB_VAR_V2 ? va[(size_t)(k - AMM_CGB_VAR_V1) * sva] : vb[(size_t)(k - AMM_CGB_VAR_V2) * svb]);
    }
    __device__ __forceinline__ double seed(int k) const { return k == seeded ? 1.0 : 0.0; }
    __device__ __forceinline__ double param(int k) const { return k < AMM_CGB_P2 ? pa[(size_t)k * sa] : pb[(size_t)(k - AMM_CGB_P2) * sb]; }
};

// the block's LDS: strip | tile [nf][256] | constants | globals | code, every part a multiple of 16 bytes
struct CgbLds {
    double2 *strip;
    double *tile, *consts, *globals;
    int *code;
};
static inline int cgb_up2(int doubles) { return (doubles + 1) & ~1; }
static int cgb_lds_bytes(const CgbArgs &A) {
    return AMM_CGB_STRIP_BYTES + 8 * (A.nf * AMM_CGB_TILE + cgb_up2(A.k1 - A.k0) + cgb_up2(A.nglobal)) + 4 * ((A.c1 - A.c0 + 3) & ~3);
}
__device__ __forceinline__ CgbLds cgb_lds(const CgbArgs &A, char *base) {
    CgbLds L;
    L.strip = reinterpret_cast<double2 *>(base);
    L.tile = reinterpret_cast<double *>(base + AMM_CGB_STRIP_BYTES);
    L.consts = L.tile + A.nf * AMM_CGB_TILE;
    L.globals = L.consts + ((A.k1 - A.k0 + 1) & ~1);
    L.code = reinterpret_cast<int *>(L.globals + ((A.nglobal + 1) & ~1));
    return L;
}
// the programs of this pass into LDS (the caller's next barrier makes them visible)
__device__ __forceinline__ void cgb_stage_programs(const CgbArgs &A, const CgbLds &L, int tid) {
    for (int k = tid; k < A.c1 - A.c0; k += AMM_CGB_BLOCK) L.code[k] = A.code[A.c0 + k];
    for (int k = tid; k < A.k1 - A.k0; k += AMM_CGB_BLOCK) L.consts[k] = A.consts[A.k0 + k];
    for (int k = tid; k < A.nglobal; k += AMM_CGB_BLOCK) L.globals[k] = A.globals[k];
}
// atoms j0 .. j0 + nt into the tile: positions, parameters, then `extra` arrays of stride n from `src` (values, or G0)
__device__ __forceinline__ void cgb_stage_tile(const CgbArgs &A, const CgbLds &L, int j0, int nt, int tid, const double *src, int extra) {
    if (tid < nt) {
        const size_t j = (size_t)j0 + tid;
        L.tile[tid] = A.pos[3 * j];
        L.tile[AMM_CGB_TILE + tid] = A.pos[3 * j + 1];
        L.tile[2 * AMM_CGB_TILE + tid] = A.pos[3 * j + 2];
        for (int p = 0; p < A.np; ++p) L.tile[(3 + p) * AMM_CGB_TILE + tid] = A.params[(size_t)p * A.n + j];
        for (int v = 0; v < extra; ++v) L.tile[(3 + A.np + v) * AMM_CGB_TILE + tid] = src[(size_t)v * A.n + j];
    }
}
__device__ __forceinline__ bool cgb_excluded(const int *idx, int e0, int e1, int j) {
    bool hit = false;
    for (int e = e0; e < e1; ++e) hit = hit || idx[e] == j;
    return hit;
}
__device__ __forceinline__ void cgb_run(const CgbArgs &A, const CgbLds &L, const CgbProg &P, const CgbLeaves &lv, double &e, double &de) {
    pexpr_run(L.code + (P.code_off - A.c0), P.ncode, L.consts + (P.const_off - A.k0), L.globals, lv, L.strip + threadIdx.x, e, de);
}

__global__ void __launch_bounds__(AMM_CGB_BLOCK) k_cgb_value(CgbArgs A) {
    extern __shared__ __align__(16) char s_cgb[];
    const CgbLds L = cgb_lds(A, s_cgb);
    const int tid = threadIdx.x;
    cgb_stage_programs(A, L, tid);
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_CGB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    const CgbProg P = A.progs[0];
    const bool with_excl = P.type == AMM_CGB_PAIR;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    int e0 = 0, e1 = 0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        if (with_excl) {
            e0 = A.excl_ptr[i];
            e1 = A.excl_ptr[i + 1];
        }
    }
    double sum = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_CGB_TILE) {
        const int nt = (A.n - j0) < AMM_CGB_TILE ? (A.n - j0) : AMM_CGB_TILE;
        __syncthreads();                    // the previous tile has been walked by every row (first trip: the programs are staged)
        cgb_stage_tile(A, L, j0, nt, tid, nullptr, 0);
        __syncthreads();
        if (!valid) continue;               // (no barrier is skipped: both are outside this test)
        for (int k = sub; k < nt; k += lpr) {
            const double dx = xi - L.tile[k], dy = yi - L.tile[AMM_CGB_TILE + k], dz = zi - L.tile[2 * AMM_CGB_TILE + k];
            const double r2 = dx * dx + dy * dy + dz * dz;
            bool part = (j0 + k != i) && (r2 < A.rc2);
            if (with_excl && part) part = !cgb_excluded(A.excl_idx, e0, e1, j0 + k);
            const double r = sqrt(part ? r2 : 1.0);
            const CgbLeaves lv{r, -1, A.params + i, A.n, L.tile + 3 * AMM_CGB_TILE + k, AMM_CGB_TILE, nullptr, 0, nullptr, 0, A.tabs};
            double e, de;
            cgb_run(A, L, P, lv, e, de);
            sum += part ? e : 0.0;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (valid && sub == 0) A.V[i] = sum;
}

__global__ void __launch_bounds__(AMM_CGB_BLOCK) k_cgb_atom(CgbArgs A) {
    extern __shared__ __align__(16) char s_cgb[];
    const CgbLds L = cgb_lds(A, s_cgb);
    const int tid = threadIdx.x;
    cgb_stage_programs(A, L, tid);
    __syncthreads();
    const int i = blockIdx.x * AMM_CGB_BLOCK + tid;
    if (i >= A.n) return;                   // (behind the kernel's only barrier)
    CgbLeaves lv{0.0, -1, A.params + i, A.n, nullptr, 0, A.V + i, A.n, nullptr, 0, A.tabs};
    for (int m = A.v0_pair ? 1 : 0; m < A.nv; ++m) {
        const CgbProg P = A.progs[m];
        double value = 0.0, e, de;
        bool ran = false;
        for (int k = 0; k < m; ++k) {
            double slope = 0.0;
            if ((P.reads >> k) & 1) {
                lv.seeded = AMM_CGB_VAR_V1 + k;
                cgb_run(A, L, P, lv, e, de);
                value = e;
                slope = de;
                ran = true;
            }
            A.J[(size_t)(4 * m + k) * A.n + i] = slope;
        }
        if (!ran) {
            lv.seeded = -1;
            cgb_run(A, L, P, lv, e, de);
            value = e;
        }
        A.V[(size_t)m * A.n + i] = value;
    }
}

template <bool EN>
__global__ void __launch_bounds__(AMM_CGB_BLOCK) k_cgb_energy(CgbArgs A) {
    extern __shared__ __align__(16) char s_cgb[];
    const CgbLds L = cgb_lds(A, s_cgb);
    const int tid = threadIdx.x;
    cgb_stage_programs(A, L, tid);
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_CGB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    int e0 = 0, e1 = 0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        if (A.any_excl) {
            e0 = A.excl_ptr[i];
            e1 = A.excl_ptr[i + 1];
        }
    }
    double fx = 0.0, fy = 0.0, fz = 0.0, esum = 0.0;
    double dV[AMM_CGB_MAX_VALUES] = {0.0, 0.0, 0.0, 0.0};         // dE/dVk_i (indexed by unrolled loops only: registers)
    for (int j0 = 0; j0 < A.n; j0 += AMM_CGB_TILE) {
        const int nt = (A.n - j0) < AMM_CGB_TILE ? (A.n - j0) : AMM_CGB_TILE;
        __syncthreads();
        cgb_stage_tile(A, L, j0, nt, tid, A.V, A.nv);
        __syncthreads();
        if (!valid) continue;
        for (int k = sub; k < nt; k += lpr) {
            const double dx = xi - L.tile[k], dy = yi - L.tile[AMM_CGB_TILE + k], dz = zi - L.tile[2 * AMM_CGB_TILE + k];
            const double r2 = dx * dx + dy * dy + dz * dz;
            const bool part0 = (j0 + k != i) && (r2 < A.rc2);
            const bool excluded = (A.any_excl && part0) ? cgb_excluded(A.excl_idx, e0, e1, j0 + k) : false;
            const double r = sqrt(part0 ? r2 : 1.0);
            CgbLeaves lv{r, 0, A.params + i, A.n, L.tile + 3 * AMM_CGB_TILE + k, AMM_CGB_TILE,
                         A.V + i, A.n, L.tile + (3 + A.np) * AMM_CGB_TILE + k, AMM_CGB_TILE, A.tabs};
            double dEdr = 0.0;
            for (int t = 0; t < A.ne; ++t) {
                const CgbProg P = A.progs[A.nv + t];
                if (P.type == AMM_CGB_SINGLE) continue;
                const bool part = part0 && !(P.type == AMM_CGB_PAIR && excluded);
                double e, de;
                lv.seeded = 0;
                cgb_run(A, L, P, lv, e, de);
                dEdr += part ? de : 0.0;
                if (EN) esum += part ? 0.5 * e : 0.0;
#pragma unroll
                for (int v = 0; v < AMM_CGB_MAX_VALUES; ++v)
                    if ((P.reads >> v) & 1) {
                        lv.seeded = AMM_CGB_VAR_V1 + v;
                        cgb_run(A, L, P, lv, e, de);
                        dV[v] += part ? de : 0.0;
                    }
            }
            const double fr = -dEdr / r;
            fx += fr * dx;
            fy += fr * dy;
            fz += fr * dz;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
#pragma unroll
        for (int v = 0; v < AMM_CGB_MAX_VALUES; ++v) dV[v] += __shfl_xor(dV[v], off);
    }
    if (valid && sub == 0) {
        // the single-particle terms, differentiated in every value they read
        CgbLeaves lv{0.0, -1, A.params + i, A.n, nullptr, 0, A.V + i, A.n, nullptr, 0, A.tabs};
        for (int t = 0; t < A.ne; ++t) {
            const CgbProg P = A.progs[A.nv + t];
            if (P.type != AMM_CGB_SINGLE) continue;
            double e = 0.0, de;
            bool ran = false;
#pragma unroll
            for (int v = 0; v < AMM_CGB_MAX_VALUES; ++v)
                if ((P.reads >> v) & 1) {
                    lv.seeded = AMM_CGB_VAR_V1 + v;
                    cgb_run(A, L, P, lv, e, de);
                    dV[v] += de;
                    ran = true;
                }
            if (EN && !ran) {
                lv.seeded = -1;
                cgb_run(A, L, P, lv, e, de);
            }
            if (EN) esum += e;
        }
        if (A.v0_pair) {
            // G^k = dE/dV^k + sum_{m > k} G^m dV^m/dV^k, down to G^0
            double G[AMM_CGB_MAX_VALUES] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = AMM_CGB_MAX_VALUES - 1; k >= 0; --k)
                if (k < A.nv) {
                    double g = dV[k];
#pragma unroll
                    for (int m = k + 1; m < AMM_CGB_MAX_VALUES; ++m)
                        if (m < A.nv) g += G[m] * A.J[(size_t)(4 * m + k) * A.n + i];
                    G[k] = g;
                }
            A.G0[i] = G[0];
            double *f = A.fdir + 3 * (size_t)i;
            f[0] = fx;
            f[1] = fy;
            f[2] = fz;
        } else {
            double *f = A.force + 3 * (size_t)i;
            if (A.accumulate) {
                f[0] += fx;
                f[1] += fy;
                f[2] += fz;
            } else {
                f[0] = fx;
                f[1] = fy;
                f[2] = fz;
            }
        }
    }
    if (EN) {
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off);
        __syncthreads();                    // every row is through with the strip: its first doubles take the wavefronts' sums
        double *red = reinterpret_cast<double *>(s_cgb);
        if ((tid & 63) == 0) red[tid >> 6] = esum;
        __syncthreads();
        if (tid == 0) A.epart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

__global__ void __launch_bounds__(AMM_CGB_BLOCK) k_cgb_chain(CgbArgs A) {
    extern __shared__ __align__(16) char s_cgb[];
    const CgbLds L = cgb_lds(A, s_cgb);
    const int tid = threadIdx.x;
    cgb_stage_programs(A, L, tid);
    const int lpr = 1 << A.lpr_shift;
    const int sub = tid & (lpr - 1);
    const int i = blockIdx.x * (AMM_CGB_BLOCK >> A.lpr_shift) + (tid >> A.lpr_shift);
    const bool valid = i < A.n;
    const CgbProg P = A.progs[0];
    const bool with_excl = P.type == AMM_CGB_PAIR;
    double xi = 0.0, yi = 0.0, zi = 0.0, g_i = 0.0;
    int e0 = 0, e1 = 0;
    if (valid) {
        xi = A.pos[3 * (size_t)i];
        yi = A.pos[3 * (size_t)i + 1];
        zi = A.pos[3 * (size_t)i + 2];
        g_i = A.G0[i];
        if (with_excl) {
            e0 = A.excl_ptr[i];
            e1 = A.excl_ptr[i + 1];
        }
    }
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += AMM_CGB_TILE) {
        const int nt = (A.n - j0) < AMM_CGB_TILE ? (A.n - j0) : AMM_CGB_TILE;
        __syncthreads();
        cgb_stage_tile(A, L, j0, nt, tid, A.G0, 1);
        __syncthreads();
        if (!valid) continue;
        for (int k = sub; k < nt; k += lpr) {
            const double dx = xi - L.tile[k], dy = yi - L.tile[AMM_CGB_TILE + k], dz = zi - L.tile[2 * AMM_CGB_TILE + k];
            const double r2 = dx * dx + dy * dy + dz * dz;
            bool part = (j0 + k != i) && (r2 < A.rc2);
            if (with_excl && part) part = !cgb_excluded(A.excl_idx, e0, e1, j0 + k);
            const double r = sqrt(part ? r2 : 1.0);
            const double *pj = L.tile + 3 * AMM_CGB_TILE + k;
            const double g_j = L.tile[(3 + A.np) * AMM_CGB_TILE + k];
            // atom i owns the sum and j is its partner; then the roles swapped
            const CgbLeaves own{r, 0, A.params + i, A.n, pj, AMM_CGB_TILE, nullptr, 0, nullptr, 0, A.tabs};
            const CgbLeaves oth{r, 0, pj, AMM_CGB_TILE, A.params + i, A.n, nullptr, 0, nullptr, 0, A.tabs};
            double e, d_own, d_oth;
            cgb_run(A, L, P, own, e, d_own);
            cgb_run(A, L, P, oth, e, d_oth);
            const double fr = part ? -(g_i * d_own + g_j * d_oth) / r : 0.0;
            fx += fr * dx;
            fy += fr * dy;
            fz += fr * dz;
        }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) {
        fx += __shfl_xor(fx, off);
        fy += __shfl_xor(fy, off);
        fz += __shfl_xor(fz, off);
    }
    if (valid && sub == 0) {
        const double *d = A.fdir + 3 * (size_t)i;
        fx += d[0];
        fy += d[1];
        fz += d[2];
        double *f = A.force + 3 * (size_t)i;
        if (A.accumulate) {
            f[0] += fx;
            f[1] += fy;
            f[2] += fz;
        } else {
            f[0] = fx;
            f[1] = fy;
            f[2] = fz;
        }
    }
}

// ---- host ----
static int cgb_fail(const char *who, const std::string &what) {
    amm_set_error(std::string(who) + ": " + what);
    return 1;
}

// the leaves a program of this place may read; sets P.reads
static int cgb_check_leaves(const char *who, const std::string &which, const int32_t *code, CgbProg &P, int place, int np, int nv) {
    const bool pair = P.type != AMM_CGB_SINGLE;
    const int own_values = place >= 0 ? place : nv;         // a value reads the values before it; an energy term all of them
    P.reads = 0;
    for (int pc = 0; pc < P.ncode; ++pc) {
        const int op = code[pc] & 0xff, arg = code[pc] >> 8;
        if (op == X_TERM_VAR) {
            const bool is_r = arg == 0 && pair;
            const bool is_v1 = arg >= AMM_CGB_VAR_V1 && arg < AMM_CGB_VAR_V1 + own_values && !(pair && place >= 0);
            const bool is_v2 = pair && place < 0 && arg >= AMM_CGB_VAR_V2 && arg < AMM_CGB_VAR_V2 + nv;
            if (!is_r && !is_v1 && !is_v2) return cgb_fail(who, which + " reads variable " + std::to_string(arg) + ", which its place does not have");
            if (is_v1) P.reads |= 1 << (arg - AMM_CGB_VAR_V1);
        } else if (op == X_TERM_P) {
            const bool ok = (arg >= 0 && arg < np) || (pair && arg >= AMM_CGB_P2 && arg < AMM_CGB_P2 + np);
            if (!ok) return cgb_fail(who, which + " reads per-particle parameter " + std::to_string(arg) + " (the force has " + std::to_string(np) + ")");
        } else if (op == X_TAB_C1 || op == X_TAB_D1 || op == X_TAB_D2) {
            if (arg < 0 || arg >= AMM_PEXPR_MAXTABLES) return cgb_fail(who, which + ": tabulated-function index out of range (limit " + std::to_string(AMM_PEXPR_MAXTABLES) + ")");
        }
    }
    return 0;
}

int amm_custom_gb_set_params_impl(amm_ctx *ctx, CustomGbForce *cg, const double *h_params, int n_params, int n_atoms) {
    if (n_params != cg->np || n_atoms != cg->n || (cg->np > 0 && !h_params))
        return cgb_fail("amm_custom_gb_set_params", "the force has " + std::to_string(cg->n) + " particles of " + std::to_string(cg->np) + " parameters, " +
                                                        std::to_string(n_atoms) + " x " + std::to_string(n_params) + " given");
    for (size_t k = 0; k < (size_t)cg->np * cg->n; ++k)
        if (!std::isfinite(h_params[k])) return cgb_fail("amm_custom_gb_set_params", "particle " + std::to_string(k % cg->n) + ": a parameter is not finite");
    AMM_HIP(hipStreamSynchronize(ctx->stream));             // nothing in flight may still read the old values
    if (cg->np > 0) AMM_HIP(hipMemcpy(cg->d_params, h_params, sizeof(double) * cg->np * cg->n, hipMemcpyHostToDevice));
    return 0;
}

int amm_custom_gb_set_globals_impl(amm_ctx *ctx, CustomGbForce *cg, const double *globals, int nglobal) {
    if (nglobal != cg->nglobal || (nglobal > 0 && !globals))
        return cgb_fail("amm_custom_gb_set_globals", "the force reads " + std::to_string(cg->nglobal) + " globals, " + std::to_string(nglobal) + " given");
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (nglobal > 0) AMM_HIP(hipMemcpy(cg->d_globals, globals, sizeof(double) * nglobal, hipMemcpyHostToDevice));
    return 0;
}

int amm_custom_gb_set_tables_impl(amm_ctx *ctx, CustomGbForce *cg, int n_tables, const int32_t *kinds, const int32_t *dims, const double *ranges,
                                  const int32_t *offsets, const double *data, int n_data) {
    const char *who = "amm_custom_gb_set_tables";
    if (n_tables < 0 || n_tables > AMM_PEXPR_MAXTABLES) return cgb_fail(who, std::to_string(n_tables) + " tabulated functions (limit " + std::to_string(AMM_PEXPR_MAXTABLES) + ")");
    if (n_tables > 0 && !kinds) return cgb_fail(who, "null argument");
    // every table word of every program finds a table of its kind
    for (int w : cg->h_code) {
        const int op = w & 0xff, arg = w >> 8;
        if (op != X_TAB_C1 && op != X_TAB_D1 && op != X_TAB_D2) continue;
        if (arg < 0 || arg >= n_tables) return cgb_fail(who, "a program reads table " + std::to_string(arg) + ": " + std::to_string(n_tables) + " given");
        const int want = op == X_TAB_C1 ? AMM_TABLE_CONTINUOUS1D : (op == X_TAB_D1 ? AMM_TABLE_DISCRETE1D : AMM_TABLE_DISCRETE2D);
        if (kinds[arg] != want) return cgb_fail(who, "table " + std::to_string(arg) + " is of kind " + std::to_string(kinds[arg]) + ", the word that reads it takes kind " + std::to_string(want));
    }
    if (amm_pair_expr_tables(ctx, cg->tabx, n_tables, kinds, dims, ranges, offsets, data, n_data)) {
        // the checks and the upload are the pair path's: its message under this entry point's name
        std::string msg = amm_last_error();
        const std::string theirs = "amm_pair_expr_set_tables";
        if (msg.compare(0, theirs.size(), theirs) == 0) msg = who + msg.substr(theirs.size());
        amm_set_error(msg);
        return 1;
    }
    return 0;
}

int amm_custom_gb_create_impl(amm_ctx *ctx, int n_params, int n_values, int n_terms, const int32_t *types, const int32_t *code,
                              const int32_t *code_ptr, const double *consts, const int32_t *const_ptr, const double *globals, int nglobal,
                              const double *h_params, const int32_t *h_excl, int n_excl, double rc, CustomGbForce **out) {
    const char *who = "amm_custom_gb_create";
    const int n = ctx->n;
    if (n > AMM_FREE_MAX_ATOMS)
        return cgb_fail(who, "a custom generalized-Born force walks all n^2 pairs up to three times and takes at most " + std::to_string(AMM_FREE_MAX_ATOMS) +
                                 " atoms (this context has " + std::to_string(n) + ")");
    if (ctx->world > 1) return cgb_fail(who, "a custom generalized-Born force (AMM_FORCE_CUSTOM_GB) runs on a single rank");
    if (n_params < 0 || n_params > AMM_TERM_MAX_PARAMS) return cgb_fail(who, std::to_string(n_params) + " per-particle parameters (limit " + std::to_string(AMM_TERM_MAX_PARAMS) + ")");
    if (n_values < 0 || n_values > AMM_CGB_MAX_VALUES) return cgb_fail(who, std::to_string(n_values) + " computed values (limit " + std::to_string(AMM_CGB_MAX_VALUES) + ")");
    if (n_terms < 0 || n_terms > AMM_CGB_MAX_TERMS) return cgb_fail(who, std::to_string(n_terms) + " energy terms (limit " + std::to_string(AMM_CGB_MAX_TERMS) + ")");
    if (nglobal < 0 || nglobal > AMM_PEXPR_MAXGLOBAL) return cgb_fail(who, std::to_string(nglobal) + " global parameters (limit " + std::to_string(AMM_PEXPR_MAXGLOBAL) + ")");
    if (!std::isfinite(rc)) return cgb_fail(who, "the cutoff is not finite");
    const int nprog = n_values + n_terms;
    CustomGbForce *cg = new CustomGbForce();
    auto bail = [&](int rc_) {
        amm_custom_gb_free(cg);
        return rc_;
    };
    cg->n = n;
    cg->np = n_params;
    cg->nv = n_values;
    cg->ne = n_terms;
    cg->nglobal = nglobal;
    cg->rc2 = rc > 0.0 ? rc * rc : std::numeric_limits<double>::infinity();
    std::memset(cg->progs, 0, sizeof(cg->progs));
    for (int p = 0; p < nprog; ++p) {
        CgbProg &P = cg->progs[p];
        const std::string which = p < n_values ? "computed value " + std::to_string(p) : "energy term " + std::to_string(p - n_values);
        P.type = types[p];
        if (P.type != AMM_CGB_SINGLE && P.type != AMM_CGB_PAIR && P.type != AMM_CGB_PAIR_NOEXCL) return bail(cgb_fail(who, which + ": unknown type " + std::to_string(P.type)));
        if (p > 0 && p < n_values && P.type != AMM_CGB_SINGLE)
            return bail(cgb_fail(who, which + " is of a pair type: only the first computed value may be a sum over pairs"));
        P.code_off = code_ptr[p];
        P.ncode = code_ptr[p + 1] - code_ptr[p];
        P.const_off = const_ptr[p];
        P.nconst = const_ptr[p + 1] - const_ptr[p];
        if (P.code_off < 0 || P.ncode < 0 || P.const_off < 0 || P.nconst < 0) return bail(cgb_fail(who, which + ": negative program offsets"));
        const std::string prefix = std::string(who) + ": " + which;
        if (amm_expr_program_validate(prefix.c_str(), code + P.code_off, P.ncode, P.nconst, nglobal, AMM_CGB_NVARS, AMM_CGB_NPARAMS, true)) return bail(1);
        if (cgb_check_leaves(who, which, code + P.code_off, P, p < n_values ? p : -1, n_params, n_values)) return bail(1);
        if (P.type == AMM_CGB_PAIR) cg->any_excl = true;
    }
    cg->v0_pair = n_values > 0 && cg->progs[0].type != AMM_CGB_SINGLE;
    if (nprog > 0) {
        cg->h_code.assign(code, code + code_ptr[nprog]);
        cg->h_consts.assign(consts, consts + const_ptr[nprog]);
    }
    for (int w : cg->h_code) {
        const int op = w & 0xff;
        if (op == X_TAB_C1 || op == X_TAB_D1 || op == X_TAB_D2) cg->uses_tables = true;
    }
    // exclusions: a symmetric CSR
    std::vector<std::vector<int>> rows(n);
    for (int e = 0; e < n_excl; ++e) {
        const int a = h_excl[2 * e], b = h_excl[2 * e + 1];
        if (a < 0 || a >= n || b < 0 || b >= n || a == b) return bail(cgb_fail(who, "exclusion " + std::to_string(e) + " (" + std::to_string(a) + ", " + std::to_string(b) + ") names no pair of particles"));
        rows[a].push_back(b);
        rows[b].push_back(a);
    }
    std::vector<int> ptr(n + 1, 0), idx;
    for (int a = 0; a < n; ++a) {
        std::sort(rows[a].begin(), rows[a].end());
        rows[a].erase(std::unique(rows[a].begin(), rows[a].end()), rows[a].end());
        idx.insert(idx.end(), rows[a].begin(), rows[a].end());
        ptr[a + 1] = (int)idx.size();
    }
    cg->tabx = new PairExpr();
    std::memset(&cg->tabx->prog.h, 0, sizeof(cg->tabx->prog.h));
    const size_t bytes = sizeof(double) * n;
    bool ok = true;
    ok = ok && hipMalloc(&cg->d_code, sizeof(int) * std::max<size_t>(cg->h_code.size(), 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_consts, sizeof(double) * std::max<size_t>(cg->h_consts.size(), 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_globals, sizeof(double) * std::max(nglobal, 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_params, bytes * std::max(n_params, 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_V, bytes * std::max(n_values, 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_J, bytes * 4 * AMM_CGB_MAX_VALUES) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_G0, bytes) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_fdir, 3 * bytes) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_excl_ptr, sizeof(int) * (n + 1)) == hipSuccess;
    ok = ok && hipMalloc(&cg->d_excl_idx, sizeof(int) * std::max<size_t>(idx.size(), 1)) == hipSuccess;
    cg->n_epart = (n + 3) / 4;          // blocks at the widest rows (64 lanes: four rows per block)
    ok = ok && hipMalloc(&cg->d_epart, sizeof(double) * cg->n_epart) == hipSuccess;
    if (!ok) return bail(cgb_fail(who, "out of device memory"));
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (!cg->h_code.empty()) AMM_HIP(hipMemcpy(cg->d_code, cg->h_code.data(), sizeof(int) * cg->h_code.size(), hipMemcpyHostToDevice));
    if (!cg->h_consts.empty()) AMM_HIP(hipMemcpy(cg->d_consts, cg->h_consts.data(), sizeof(double) * cg->h_consts.size(), hipMemcpyHostToDevice));
    AMM_HIP(hipMemcpy(cg->d_excl_ptr, ptr.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice));
    if (!idx.empty()) AMM_HIP(hipMemcpy(cg->d_excl_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
    AMM_HIP(hipMemset(cg->d_J, 0, bytes * 4 * AMM_CGB_MAX_VALUES));
    if (amm_custom_gb_set_globals_impl(ctx, cg, globals, nglobal)) return bail(1);
    if (amm_custom_gb_set_params_impl(ctx, cg, h_params, n_params, n)) return bail(1);
    *out = cg;
    return 0;
}

// lanes per row (the context's option, or free.hip's choice from n), as a shift; the blocks that cover n rows with it
static int cgb_geometry(amm_ctx *ctx, int n, int &nblocks) {
    const int lpr = ctx->opt_cgb_lpr > 0 ? ctx->opt_cgb_lpr : amm_free_lanes_per_row(n);
    int shift = 0;
    while ((1 << shift) < lpr) ++shift;
    const int rows_per_block = AMM_CGB_BLOCK >> shift;
    nblocks = (n + rows_per_block - 1) / rows_per_block;
    return shift;
}

// the arguments of one pass: the programs first .. last (exclusive) are staged; `extra` doubles per atom follow the parameters in the tile
static CgbArgs cgb_args(CustomGbForce *cg, int shift, const double *d_pos, double *d_force, int accumulate, int first, int last, int extra) {
    CgbArgs A;
    std::memset(&A, 0, sizeof(A));
    A.n = cg->n;
    A.lpr_shift = shift;
    A.accumulate = accumulate;
    A.np = cg->np;
    A.nv = cg->nv;
    A.ne = cg->ne;
    A.v0_pair = cg->v0_pair ? 1 : 0;
    A.nglobal = cg->nglobal;
    A.any_excl = cg->any_excl ? 1 : 0;
    if (last > first) {
        A.c0 = cg->progs[first].code_off;
        A.c1 = cg->progs[last - 1].code_off + cg->progs[last - 1].ncode;
        A.k0 = cg->progs[first].const_off;
        A.k1 = cg->progs[last - 1].const_off + cg->progs[last - 1].nconst;
    }
    A.nf = extra < 0 ? 0 : 3 + cg->np + extra;
    A.pos = d_pos;
    A.params = cg->d_params;
    A.V = cg->d_V;
    A.J = cg->d_J;
    A.G0 = cg->d_G0;
    A.fdir = cg->d_fdir;
    A.force = d_force;
    A.epart = cg->d_epart;
    A.excl_ptr = cg->d_excl_ptr;
    A.excl_idx = cg->d_excl_idx;
    A.code = cg->d_code;
    A.consts = cg->d_consts;
    A.globals = cg->d_globals;
    A.tabs = cg->tabx->d_tabs;
    A.rc2 = cg->rc2;
    std::memcpy(A.progs, cg->progs, sizeof(A.progs));
    return A;
}

template <class K>
static int cgb_launch(amm_ctx *ctx, CustomGbForce *cg, int which, K kern, int nblocks, const CgbArgs &A) {
    const int lds = cgb_lds_bytes(A);
    if (lds > 160 * 1024) return cgb_fail("custom generalized-Born force", "the pass needs " + std::to_string(lds) + " bytes of LDS");       // (cannot happen: 104 KiB at the limits)
    static bool lds_set[16][5] = {{false}};     // per device and kernel: the attribute is set once, to all a block may have
    const int dev = ctx->device & 15;
    if (!lds_set[dev][which]) {
        AMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_set[dev][which] = true;
    }
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(AMM_CGB_BLOCK), (size_t)lds, ctx->stream, A);
    return 0;
}

// passes 1 and 2: the computed values at d_pos
static int cgb_values(amm_ctx *ctx, CustomGbForce *cg, const double *d_pos, int shift, int nblocks) {
    if (cg->uses_tables && !cg->tabx->d_tabs)
        return cgb_fail("custom generalized-Born force (AMM_FORCE_CUSTOM_GB)", "the programs read tabulated functions and none are set: amm_custom_gb_set_tables");
    if (cg->v0_pair && cgb_launch(ctx, cg, 0, k_cgb_value, nblocks, cgb_args(cg, shift, d_pos, nullptr, 0, 0, 1, 0))) return 1;
    const int first = cg->v0_pair ? 1 : 0;
    if (cg->nv > first &&
        cgb_launch(ctx, cg, 1, k_cgb_atom, (cg->n + AMM_CGB_BLOCK - 1) / AMM_CGB_BLOCK, cgb_args(cg, 0, d_pos, nullptr, 0, first, cg->nv, -1)))
        return 1;
    return 0;
}

int amm_custom_gb_eval_impl(amm_ctx *ctx, CustomGbForce *cg, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    int nblocks = 0;
    const int shift = cgb_geometry(ctx, cg->n, nblocks);
    const bool en = d_energy != nullptr;
    if (en && cg->n_epart < nblocks) return cgb_fail("custom generalized-Born force", "more blocks than energy partials");      // (cannot happen: sized for 64 lanes per row)
    if (cgb_values(ctx, cg, d_pos, shift, nblocks)) return 1;
    const CgbArgs E = cgb_args(cg, shift, d_pos, d_force, accumulate, cg->nv, cg->nv + cg->ne, cg->nv);
    if (en ? cgb_launch(ctx, cg, 2, k_cgb_energy<true>, nblocks, E) : cgb_launch(ctx, cg, 3, k_cgb_energy<false>, nblocks, E)) return 1;
    if (cg->v0_pair && cgb_launch(ctx, cg, 4, k_cgb_chain, nblocks, cgb_args(cg, shift, d_pos, d_force, accumulate, 0, 1, 1))) return 1;
    AMM_HIP(hipGetLastError());
    cg->n_evals++;
    if (en) return amm_reduce_add(ctx, cg->d_epart, nblocks, 1.0, d_energy);
    return 0;
}

int amm_custom_gb_values_impl(amm_ctx *ctx, CustomGbForce *cg, const double *d_pos, double *h_out) {
    int nblocks = 0;
    const int shift = cgb_geometry(ctx, cg->n, nblocks);
    if (cgb_values(ctx, cg, d_pos, shift, nblocks)) return 1;
    AMM_HIP(hipGetLastError());
    AMM_HIP(hipStreamSynchronize(ctx->stream));
    if (cg->nv > 0) AMM_HIP(hipMemcpy(h_out, cg->d_V, sizeof(double) * cg->nv * cg->n, hipMemcpyDeviceToHost));
    return 0;
}

void amm_custom_gb_free(CustomGbForce *cg) {
    if (!cg) return;
    void *arrays[] = {cg->d_code, cg->d_consts, cg->d_globals, cg->d_params, cg->d_V, cg->d_J, cg->d_G0, cg->d_fdir, cg->d_excl_ptr, cg->d_excl_idx, cg->d_epart};
    for (void *a : arrays)
        if (a) (void)hipFree(a);
    amm_pair_expr_free(cg->tabx);
    delete cg;
}
