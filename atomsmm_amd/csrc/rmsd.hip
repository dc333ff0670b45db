// atomsmm_amd/csrc/rmsd.hip -- RMSDForce (AMM_FORCE_RMSD): the root-mean-square deviation of N selected particles from reference
// coordinates after the optimal rigid superposition, as an energy (nm) and its gradient.
//
//   c = sum x_i / N;  y'_i = the reference, centred once on the host in extended precision;  M = sum y'_i x_i^T (x needs no centring
//   because sum y' = 0);  R = the proper rotation of Horn's quaternion for M (rmsd_fit.h);  d_i = x_i - c - R y'_i;
//   energy = rmsd = sqrt(sum |d_i|^2 / N);  force on i = -d_i / (N rmsd)  (R is stationary: its derivative does not enter).
//   sum |d_i|^2 / N < 1e-20 nm^2: energy 0 and zero rows -- defined, never a NaN.
// Positions are read raw: no box, no minimum image.  The energy comes from the residual itself: (sum |x - c|^2 + sum |y'|^2 -
// 2 lambda_max) / N cancels to 1e-6 relative at rmsd = 1.7e-4 nm, the residual does not.
//
// fp64, fixed order of summation everywhere, no atomics, no counters: the same positions give the same bits.  A reduction is a
// strided walk per lane, a __shfl_xor butterfly per wavefront and the wavefronts' partials from LDS in wavefront order.
//
// One block (k_rmsd_one, 1024 lanes), one launch: the twelve sums; the fit on lane 0; the residuals, parked per particle in
// d_res, and their sum of squares; the force rows.  Several blocks, three launches of 256 lanes, block b owning the particles
// [b chunk, (b + 1) chunk): k_rmsd_sums leaves twelve partial sums per block; k_rmsd_resid adds them in block order and fits in
// EVERY block (no grid-wide wait), parks the residuals of its chunk and leaves their sum of squares; k_rmsd_rows adds those in
// block order and writes the rows.  When the evaluation does not accumulate, the rows of the particles outside the selection are
// cleared by further blocks of the launch that writes the rows (a list of them is kept): they touch no row of the selection.
// RMSD_AUTO_SINGLE is where the library changes from the one to the other (measured: below, and DESIGN.md 3.RM).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "amm_ctx.h"
#include "device_utils.h"
#include "rmsd_fit.h"

#define RMSD_ONE_BLOCK 1024         // lanes of the single block
#define RMSD_BLOCK 256              // lanes of a block of the three-launch path
#define RMSD_MAX_BLOCKS 1024        // ... whose partials one lane per sum adds up in order
#define RMSD_PER_BLOCK 1024         // particles per block when the library chooses the number of blocks
// option rmsd_blocks = 0: selections up to this size take the single block.  Measured on an MI355X (profiles/rmsd_cost.txt, us per
// evaluation, one block / blocks): N = 64 18.6 / 17.3, 1 024 20.5 / 19.1, 2 048 22.0 / 20.2, 4 096 25.5 / 20.5, 8 192 33.3 / 21.2,
// 16 384 50.8 / 25.0, 98 304 263.3 / 47.0.  Up to 2 048 the two are within 1.8 us of each other -- the fit on one lane, about 9 us, is
// most of either, and the kernel trace gives 17.4 us for the one launch against 15.1 us for the three plus their two boundaries --
// so the path with two launches fewer is taken; from 4 096 on the blocks win by a fifth and more.
#define RMSD_AUTO_SINGLE 2048
#define RMSD_ZERO_ROWS 4            // rows a lane of a clearing block writes
#define RMSD_GUARD 1e-20            // nm^2: mean square deviations below it are zero

struct RmsdForce {
    int n_sel = 0, n_other = 0;
    int blocks_opt = 0;                 // the context's rmsd_blocks when the force was created
    int n_blocks = 1, chunk = 0;        // the path taken: 1 = single block; else blocks and particles per block
    int *d_idx = nullptr;               // [n_sel] the selected particles, in the caller's order
    int *d_other = nullptr;             // [n_other] the other particles, ascending
    double *d_ref = nullptr;            // [n_sel][3] centred reference rows of the selected particles
    double *d_res = nullptr;            // [n_sel][3] residuals d_i of the evaluation in flight
    double *d_part = nullptr;           // [n_blocks][12] partial sums
    double *d_rpart = nullptr;          // [n_blocks] partial sums of |d|^2
    bool ready = false;                 // the arrays above stand (false after a reload that ran out of device memory)
    long long launches = 0;
};

struct RmsdArgs {
    int n_sel, n_other, n_blocks, chunk, accumulate;
    const int *idx, *other;
    const double *ref, *pos;
    double *res, *part, *rpart, *force, *energy;
};

// K sums over the block in a fixed order: butterfly per wavefront, then lane k < K adds the wavefronts' partials in wavefront order.
// s_wave: [T / 64][K]; the totals land in s_out[K]; every lane of the block calls (two barriers inside).
template <int K, int T>
__device__ __forceinline__ void rmsd_block_sum(double (&s)[K], double *s_wave, double *s_out) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_wave[(tid >> 6) * K + k] = s[k];
    }
    __syncthreads();
    if (tid < K) {
        double acc = s_wave[tid];
        for (int w = 1; w < T / 64; ++w) acc += s_wave[w * K + tid];
        s_out[tid] = acc;
    }
    __syncthreads();
}

// the twelve sums of the particles lo, lo + T, ... < hi of this lane
template <int T>
__device__ __forceinline__ void rmsd_walk_sums(const RmsdArgs &A, int lo, int hi, double (&s)[12]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += T) {
        const int a = A.idx[i];
        const double x0 = A.pos[3 * (size_t)a], x1 = A.pos[3 * (size_t)a + 1], x2 = A.pos[3 * (size_t)a + 2];
        const double y0 = A.ref[3 * (size_t)i], y1 = A.ref[3 * (size_t)i + 1], y2 = A.ref[3 * (size_t)i + 2];
        s[0] += x0;
        s[1] += x1;
        s[2] += x2;
        s[3] += y0 * x0;
        s[4] += y0 * x1;
        s[5] += y0 * x2;
        s[6] += y1 * x0;
        s[7] += y1 * x1;
        s[8] += y1 * x2;
        s[9] += y2 * x0;
        s[10] += y2 * x1;
        s[11] += y2 * x2;
    }
}

// residuals of this lane's particles into A.res; returns the lane's sum of their squares
template <int T>
__device__ __forceinline__ double rmsd_walk_resid(const RmsdArgs &A, int lo, int hi, const double *fit) {
#pragma clang fp contract(off)
    const double c0 = fit[0], c1 = fit[1], c2 = fit[2];
    const double r00 = fit[3], r01 = fit[4], r02 = fit[5], r10 = fit[6], r11 = fit[7], r12 = fit[8], r20 = fit[9], r21 = fit[10], r22 = fit[11];
    double ss = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += T) {
        const int a = A.idx[i];
        const double x0 = A.pos[3 * (size_t)a], x1 = A.pos[3 * (size_t)a + 1], x2 = A.pos[3 * (size_t)a + 2];
        const double y0 = A.ref[3 * (size_t)i], y1 = A.ref[3 * (size_t)i + 1], y2 = A.ref[3 * (size_t)i + 2];
        const double d0 = (x0 - c0) - ((r00 * y0 + r01 * y1) + r02 * y2);
        const double d1 = (x1 - c1) - ((r10 * y0 + r11 * y1) + r12 * y2);
        const double d2 = (x2 - c2) - ((r20 * y0 + r21 * y1) + r22 * y2);
        A.res[3 * (size_t)i] = d0;
        A.res[3 * (size_t)i + 1] = d1;
        A.res[3 * (size_t)i + 2] = d2;
        ss += (d0 * d0 + d1 * d1) + d2 * d2;
    }
    return ss;
}

// the rows of this lane's particles from the residuals it parked itself (the same lane, the same stride: no barrier in between)
template <int T>
__device__ __forceinline__ void rmsd_walk_rows(const RmsdArgs &A, int lo, int hi, double sum_sq) {
#pragma clang fp contract(off)
    const double msd = sum_sq / (double)A.n_sel;
    const bool zero = msd < RMSD_GUARD;                  // (positions that are not numbers stay visible: they are no deviation of zero)
    const double rmsd = zero ? 0.0 : sqrt(msd);
    const double scale = zero ? 0.0 : -1.0 / ((double)A.n_sel * rmsd);
    for (int i = lo + (int)threadIdx.x; i < hi; i += T) {
        const int a = A.idx[i];
        if (zero) {
            if (!A.accumulate) store_force_row(A.force, a, 0.0, 0.0, 0.0, 0);
        }
        else store_force_row(A.force, a, scale * A.res[3 * (size_t)i], scale * A.res[3 * (size_t)i + 1], scale * A.res[3 * (size_t)i + 2], A.accumulate);
    }
    if (A.energy && blockIdx.x == 0 && threadIdx.x == 0) *A.energy += rmsd;
}

// block `zb` of `nzb` clearing blocks: the rows of the particles outside the selection
template <int T>
__device__ __forceinline__ void rmsd_clear_rows(const RmsdArgs &A, int zb, int nzb) {
    for (long j = (long)zb * T + threadIdx.x; j < (long)A.n_other; j += (long)nzb * T) {
        const int a = A.other[j];
        store_force_row(A.force, a, 0.0, 0.0, 0.0, 0);
    }
}

__global__ void __launch_bounds__(RMSD_ONE_BLOCK) k_rmsd_one(RmsdArgs A) {
#pragma clang fp contract(off)
    constexpr int T = RMSD_ONE_BLOCK;
    if (blockIdx.x > 0) {
        rmsd_clear_rows<T>(A, blockIdx.x - 1, gridDim.x - 1);
        return;
    }
    __shared__ double s_wave[(T / 64) * 12], s_sums[12], s_fit[12], s_ss[1];
    double s[12];
    rmsd_walk_sums<T>(A, 0, A.n_sel, s);
    rmsd_block_sum<12, T>(s, s_wave, s_sums);
    if (threadIdx.x == 0) amm_rmsd_fit(s_sums, A.n_sel, s_fit);
    __syncthreads();
    double ss[1];
    ss[0] = rmsd_walk_resid<T>(A, 0, A.n_sel, s_fit);
    rmsd_block_sum<1, T>(ss, s_wave, s_ss);
    rmsd_walk_rows<T>(A, 0, A.n_sel, s_ss[0]);
}

__global__ void __launch_bounds__(RMSD_BLOCK) k_rmsd_sums(RmsdArgs A) {
#pragma clang fp contract(off)
    constexpr int T = RMSD_BLOCK;
    __shared__ double s_wave[(T / 64) * 12], s_sums[12];
    const int lo = min((int)blockIdx.x * A.chunk, A.n_sel), hi = min(lo + A.chunk, A.n_sel);
    double s[12];
    rmsd_walk_sums<T>(A, lo, hi, s);
    rmsd_block_sum<12, T>(s, s_wave, s_sums);
    if (threadIdx.x < 12) A.part[(size_t)blockIdx.x * 12 + threadIdx.x] = s_sums[threadIdx.x];
}

__global__ void __launch_bounds__(RMSD_BLOCK) k_rmsd_resid(RmsdArgs A) {
#pragma clang fp contract(off)
    constexpr int T = RMSD_BLOCK;
    __shared__ double s_wave[T / 64], s_sums[12], s_fit[12], s_ss[1];
    if (threadIdx.x < 12) {
        double acc = A.part[threadIdx.x];
        for (int b = 1; b < A.n_blocks; ++b) acc += A.part[(size_t)b * 12 + threadIdx.x];
        s_sums[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) amm_rmsd_fit(s_sums, A.n_sel, s_fit);
    __syncthreads();
    const int lo = min((int)blockIdx.x * A.chunk, A.n_sel), hi = min(lo + A.chunk, A.n_sel);
    double ss[1];
    ss[0] = rmsd_walk_resid<T>(A, lo, hi, s_fit);
    rmsd_block_sum<1, T>(ss, s_wave, s_ss);
    if (threadIdx.x == 0) A.rpart[blockIdx.x] = s_ss[0];
}

__global__ void __launch_bounds__(RMSD_BLOCK) k_rmsd_rows(RmsdArgs A) {
#pragma clang fp contract(off)
    constexpr int T = RMSD_BLOCK;
    if ((int)blockIdx.x >= A.n_blocks) {
        rmsd_clear_rows<T>(A, blockIdx.x - A.n_blocks, gridDim.x - A.n_blocks);
        return;
    }
    __shared__ double s_ss[1];
    if (threadIdx.x == 0) {
        double acc = A.rpart[0];
        for (int b = 1; b < A.n_blocks; ++b) acc += A.rpart[b];
        s_ss[0] = acc;
    }
    __syncthreads();
    const int lo = min((int)blockIdx.x * A.chunk, A.n_sel), hi = min(lo + A.chunk, A.n_sel);
    rmsd_walk_rows<T>(A, lo, hi, s_ss[0]);
}

int amm_rmsd_eval_impl(amm_ctx *ctx, RmsdForce *rf, const double *d_pos, double *d_force, int accumulate, double *d_energy) {
    if (!rf->ready) {
        amm_set_error("evaluation of an RMSD force (AMM_FORCE_RMSD) whose last amm_rmsd_set_reference failed");
        return 1;
    }
    RmsdArgs A;
    A.n_sel = rf->n_sel;
    A.n_other = rf->n_other;
    A.n_blocks = rf->n_blocks;
    A.chunk = rf->chunk;
    A.accumulate = accumulate ? 1 : 0;
    A.idx = rf->d_idx;
    A.other = rf->d_other;
    A.ref = rf->d_ref;
    A.pos = d_pos;
    A.res = rf->d_res;
    A.part = rf->d_part;
    A.rpart = rf->d_rpart;
    A.force = d_force;
    A.energy = d_energy;
    if (rf->n_blocks == 1) {
        const int per = RMSD_ONE_BLOCK * RMSD_ZERO_ROWS;
        const int clear = accumulate || rf->n_other == 0 ? 0 : std::min(1024, (rf->n_other + per - 1) / per);
        hipLaunchKernelGGL(k_rmsd_one, dim3(1 + clear), dim3(RMSD_ONE_BLOCK), 0, ctx->stream, A);
        AMM_HIP(hipGetLastError());
        rf->launches += 1;
        return 0;
    }
    const int per = RMSD_BLOCK * RMSD_ZERO_ROWS;
    const int clear = accumulate || rf->n_other == 0 ? 0 : std::min(4096, (rf->n_other + per - 1) / per);
    hipLaunchKernelGGL(k_rmsd_sums, dim3(rf->n_blocks), dim3(RMSD_BLOCK), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rmsd_resid, dim3(rf->n_blocks), dim3(RMSD_BLOCK), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rmsd_rows, dim3(rf->n_blocks + clear), dim3(RMSD_BLOCK), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    rf->launches += 3;
    return 0;
}

// ---- host ----
static void rmsd_free_arrays(RmsdForce *rf) {
    for (void *p : {(void *)rf->d_idx, (void *)rf->d_other, (void *)rf->d_ref, (void *)rf->d_res, (void *)rf->d_part, (void *)rf->d_rpart})
        if (p) (void)hipFree(p);
    rf->d_idx = rf->d_other = nullptr;
    rf->d_ref = rf->d_res = rf->d_part = rf->d_rpart = nullptr;
}

// checks the selection, centres the reference and (re)builds the device arrays of `rf`; `who` names the entry point
static int rmsd_load(amm_ctx *ctx, RmsdForce *rf, const char *who, const int32_t *h_particles, int n_sel, const double *h_ref) {
    auto fail = [who](const std::string &what) {
        amm_set_error(std::string(who) + ": " + what + " (AMM_FORCE_RMSD)");
        return 1;
    };
    const int n = ctx->n;
    if (n_sel < 1) return fail("a selection of " + std::to_string(n_sel) + " particles: the deviation needs at least one");
    if (ctx->world > 1) return fail("an RMSD force runs on a single rank");
    std::vector<char> taken(n, 0);
    for (int i = 0; i < n_sel; ++i) {
        const int a = h_particles[i];
        if (a < 0 || a >= n) return fail("particle index " + std::to_string(a) + " (entry " + std::to_string(i) + ") is out of range");
        if (taken[a]) return fail("particle " + std::to_string(a) + " is listed twice");
        taken[a] = 1;
    }
    for (size_t k = 0; k < (size_t)n_sel * 3; ++k)
        if (!std::isfinite(h_ref[k])) return fail("reference coordinate " + std::to_string(k % 3) + " of entry " + std::to_string(k / 3) + " is not finite");
    // the reference, centred in extended precision
    long double mean[3] = {0.0L, 0.0L, 0.0L};
    for (int i = 0; i < n_sel; ++i)
        for (int x = 0; x < 3; ++x) mean[x] += (long double)h_ref[3 * (size_t)i + x];
    for (int x = 0; x < 3; ++x) mean[x] /= (long double)n_sel;
    std::vector<double> ref((size_t)n_sel * 3);
    for (int i = 0; i < n_sel; ++i)
        for (int x = 0; x < 3; ++x) ref[3 * (size_t)i + x] = (double)((long double)h_ref[3 * (size_t)i + x] - mean[x]);
    std::vector<int> other;
    other.reserve(n - n_sel);
    for (int a = 0; a < n; ++a)
        if (!taken[a]) other.push_back(a);
    int blocks = rf->blocks_opt;
    if (blocks == 0) blocks = n_sel <= RMSD_AUTO_SINGLE ? 1 : std::min(RMSD_MAX_BLOCKS, (n_sel + RMSD_PER_BLOCK - 1) / RMSD_PER_BLOCK);
    AMM_HIP(hipSetDevice(ctx->device));
    AMM_HIP(hipStreamSynchronize(ctx->stream));            // nothing in flight may still read the old arrays
    rmsd_free_arrays(rf);
    rf->ready = false;
    rf->n_sel = n_sel;
    rf->n_other = (int)other.size();
    rf->n_blocks = blocks;
    rf->chunk = (n_sel + blocks - 1) / blocks;
    if (amm_upload(&rf->d_idx, h_particles, (size_t)n_sel)) return 1;
    if (amm_upload(&rf->d_other, other.data(), other.size())) return 1;
    if (amm_upload(&rf->d_ref, ref.data(), ref.size())) return 1;
    AMM_HIP(hipMalloc(&rf->d_res, sizeof(double) * 3 * (size_t)n_sel));
    AMM_HIP(hipMalloc(&rf->d_part, sizeof(double) * 12 * (size_t)blocks));
    AMM_HIP(hipMalloc(&rf->d_rpart, sizeof(double) * (size_t)blocks));
    AMM_HIP(hipMemset(rf->d_res, 0, sizeof(double) * 3 * (size_t)n_sel));
    AMM_HIP(hipMemset(rf->d_part, 0, sizeof(double) * 12 * (size_t)blocks));
    AMM_HIP(hipMemset(rf->d_rpart, 0, sizeof(double) * (size_t)blocks));
    rf->ready = true;
    return 0;
}

int amm_rmsd_create_impl(amm_ctx *ctx, const int32_t *h_particles, int n_sel, const double *h_ref, RmsdForce **out) {
    RmsdForce *rf = new RmsdForce();
    rf->blocks_opt = ctx->opt_rmsd_blocks;
    if (rmsd_load(ctx, rf, "amm_rmsd_create", h_particles, n_sel, h_ref)) {
        amm_rmsd_free(rf);
        return 1;
    }
    *out = rf;
    return 0;
}

// a refused call leaves the force as it was: the checks come before anything is freed
int amm_rmsd_set_reference_impl(amm_ctx *ctx, RmsdForce *rf, const int32_t *h_particles, int n_sel, const double *h_ref) {
    return rmsd_load(ctx, rf, "amm_rmsd_set_reference", h_particles, n_sel, h_ref);
}

int amm_rmsd_stats_impl(RmsdForce *rf, int64_t out[4]) {
    out[0] = rf->n_sel;
    out[1] = rf->n_blocks;
    out[2] = rf->n_blocks == 1 ? 1 : 3;
    out[3] = rf->launches;
    return 0;
}

void amm_rmsd_free(RmsdForce *rf) {
    if (!rf) return;
    rmsd_free_arrays(rf);
    delete rf;
}
