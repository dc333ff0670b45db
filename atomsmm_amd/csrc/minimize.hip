// atomsmm_amd/csrc/minimize.hip -- vector work of the L-BFGS energy minimiser (gfx950, fp64).
//
// The reference reaches OpenMM's LocalEnergyMinimizer::minimize through app.Simulation.minimizeEnergy; OpenMM runs liblbfgs on
// the host over positions it downloads and uploads at every evaluation.  Here the positions, the gradients and the whole L-BFGS
// history stay on the device and the host sees one block of eight scalars per energy evaluation.
//
// Vector-free (Gram-matrix) form of the two-loop recursion (Chen, Wang, Zhou: "Large-scale L-BFGS using MapReduce", NIPS 2014).
// The basis is b = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g]: a ring of [2m][3N] doubles and the current gradient.  The search direction
// is d = sum_j delta_j b_j, and the two-loop recursion that yields delta needs nothing but the (2m+1) x (2m+1) dot products
// b_i . b_j.  One iteration brings three new vectors (s_k, y_k, g_{k+1}), hence three new rows and columns of that matrix:
//   k_min_gram     forms s = x - x_prev and y = g - g_prev into the ring slot, reads every basis vector ONCE and leaves the
//                  3 (2m+1) new dot products, g.g and max|g| (the convergence test: the host never reads the gradient);
//   k_min_coef     one wavefront: curvature guard, two-loop recursion on the matrix, delta and g.d;
//   k_min_combine  d = sum_j delta_j b_j, every basis vector read once, and the largest displacement of an atom along d;
//   k_min_trial    x = x_prev + alpha d with alpha cut down so that no atom moves farther than max_step; atoms of mass 0 stay.
// Sums are fixed-order: per-thread strided sums, a shuffle butterfly per wavefront, four wavefronts in order, then the block that
// draws the last ticket adds the blocks' partial sums in index order (device_utils.h: amm_last_block) -- the same bits on every
// launch.  The two maxima are order-independent by nature.
#include <cmath>

#include "amm_ctx.h"
#include "device_utils.h"

#define AMM_MIN_MAXM 8                       // largest memory (pairs kept)
#define AMM_MIN_NB (2 * AMM_MIN_MAXM + 1)    // basis vectors at that memory: s_j -> j, y_j -> AMM_MIN_MAXM + j, g -> 2 AMM_MIN_MAXM
#define AMM_MIN_NV (3 * AMM_MIN_NB + 1)      // values a Gram update reduces: three rows + max|g|
#define AMM_MIN_NVP 64                       // ... padded to a wavefront
#define AMM_MIN_MAXBLOCKS 512
#define AMM_MIN_CURVATURE 1e-10              // a pair with s.y <= this |s| |y| is dropped

// istate (device ints): [0 .. 8) valid[j] of ring slot j, [16] pairs dropped so far, [17] resets to steepest descent (g.d >= 0)
#define AMM_MIN_I_DROPPED 16
#define AMM_MIN_I_RESETS 17
#define AMM_MIN_ISTATE 32

struct MinObj {
    int n = 0, m = 0;
    double max_step = 0.1, sign = 1.0;       // sign -1: the caller's "gradients" are forces (amm_force_eval output)
    const double *d_mass = nullptr;          // caller-owned, may be null (every atom free)
    double *d_scal = nullptr;                // caller-owned block of 8 doubles (include/atomsmm_hip.h: amm_min_create)
    double *d_ring = nullptr, *d_xprev = nullptr, *d_gprev = nullptr, *d_dir = nullptr;
    double *d_gram = nullptr, *d_delta = nullptr, *d_part = nullptr;
    int *d_istate = nullptr, *d_ticket = nullptr;
    int head = 0;                            // ring slot the next pair goes to
    bool begun = false;
    long long n_advances = 0, n_trials = 0, n_restarts = 0;
};

struct MinGramArgs {
    long long n3;
    int m, p, form;
    double sign;
    const double *x, *g, *mass;
    double *ring, *xprev, *gprev, *part, *gram, *scal;
    int *ticket;
};

static __device__ __forceinline__ double min_ld(const double *p) {
    return __longlong_as_double((long long)amm_ld_l2((const unsigned long long *)p));
}

// Gram update.  form = 1: the pair (s, y) = (x - x_prev, g - g_prev) goes to ring slot p; form = 0 (first gradient after
// amm_min_begin): no pair, only the products of g.  Either way x_prev <- x, g_prev <- g (the gradient of an atom of mass 0 counts
// as zero from here on: such an atom has no s, no y and no share in d).
__global__ void __launch_bounds__(256) k_min_gram(MinGramArgs A) {
    constexpr int MM = AMM_MIN_MAXM, NB = AMM_MIN_NB;
    double acc[3][NB];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[r][c] = 0.0;
    double gmax = 0.0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n3; i += stride) {
        const bool is_free = !A.mass || A.mass[i / 3] > 0.0;
        const double x = A.x[i];
        const double g = is_free ? A.sign * A.g[i] : 0.0;
        double s = 0.0, y = 0.0;
        if (A.form && is_free) {
            s = x - A.xprev[i];
            y = g - A.gprev[i];
        }
        double bs[MM], by[MM];
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            bs[j] = by[j] = 0.0;
            if (A.form && j < A.m) {
                bs[j] = j == A.p ? s : A.ring[(long long)j * A.n3 + i];
                by[j] = j == A.p ? y : A.ring[(long long)(A.m + j) * A.n3 + i];
            }
        }
        if (A.form) {
            A.ring[(long long)A.p * A.n3 + i] = s;
            A.ring[(long long)(A.m + A.p) * A.n3 + i] = y;
        }
        A.xprev[i] = x;
        A.gprev[i] = g;
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            acc[0][j] += s * bs[j];
            acc[0][MM + j] += s * by[j];
            acc[1][j] += y * bs[j];
            acc[1][MM + j] += y * by[j];
            acc[2][j] += g * bs[j];
            acc[2][MM + j] += g * by[j];
        }
        acc[0][2 * MM] += s * g;
        acc[1][2 * MM] += y * g;
        acc[2][2 * MM] += g * g;
        gmax = fmax(gmax, fabs(g));
    }
    // block partials: butterfly per wavefront, the four wavefronts in order
    __shared__ double red[4][AMM_MIN_NVP];
    __shared__ double fin[4][AMM_MIN_NVP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            double v = acc[r][c];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) red[w][r * NB + c] = v;
        }
    for (int off = 32; off > 0; off >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, off));
    if (lane == 0) red[w][AMM_MIN_NV - 1] = gmax;
    __syncthreads();
    if (threadIdx.x < AMM_MIN_NV) {
        const int v = threadIdx.x;
        const double sum = v == AMM_MIN_NV - 1 ? fmax(fmax(red[0][v], red[1][v]), fmax(red[2][v], red[3][v]))
                                               : ((red[0][v] + red[1][v]) + red[2][v]) + red[3][v];
        // (through L2: the last block reads it)
        amm_st_l2((unsigned long long *)&A.part[(long long)blockIdx.x * AMM_MIN_NVP + v], (unsigned long long)__double_as_longlong(sum));
    }
    if (!amm_last_block(A.ticket)) return;
    // ---- last block: the blocks' partials in index order (wavefront w takes the w-th quarter of the blocks, then the quarters in order)
    const int nblk = (int)gridDim.x, per = (nblk + 3) / 4;
    const int b0 = min(w * per, nblk), b1 = min(b0 + per, nblk);
    double tot = 0.0;
    if (lane < AMM_MIN_NV) {
        if (lane == AMM_MIN_NV - 1) {
            for (int b = b0; b < b1; ++b) tot = fmax(tot, min_ld(&A.part[(long long)b * AMM_MIN_NVP + lane]));
        } else {
#pragma unroll 8
            for (int b = b0; b < b1; ++b) tot += min_ld(&A.part[(long long)b * AMM_MIN_NVP + lane]);
        }
    }
    fin[w][lane] = tot;
    __syncthreads();
    if (threadIdx.x < AMM_MIN_NV) {
        const int v = threadIdx.x;
        const double sum = v == AMM_MIN_NV - 1 ? fmax(fmax(fin[0][v], fin[1][v]), fmax(fin[2][v], fin[3][v]))
                                               : ((fin[0][v] + fin[1][v]) + fin[2][v]) + fin[3][v];
        if (v == AMM_MIN_NV - 1) {
            A.scal[3] = sum;
        } else {
            const int r = v / NB, c = v - r * NB;
            const int row = r == 0 ? A.p : (r == 1 ? MM + A.p : 2 * MM);
            if (r == 2 || A.form) {          // (symmetric entries get the same bits from both of their sums: same products, same order)
                A.gram[row * NB + c] = sum;
                A.gram[c * NB + row] = sum;
            }
            if (r == 2 && c == 2 * MM) A.scal[2] = sum;
        }
    }
}

// Coefficients: ONE wavefront, lane j holds delta_j.  newest: ring slot of the pair the Gram update has just formed (form = 1).
// scal[1] <- g.d, scal[4] <- 1 if that pair was dropped, scal[5] <- pairs in use, scal[7] <- 0 (k_min_combine's maximum).
__global__ void __launch_bounds__(64) k_min_coef(int m, int newest, int form, const double *gram, double *delta, double *scal, int *istate) {
    constexpr int MM = AMM_MIN_MAXM, NB = AMM_MIN_NB;
    __shared__ double sG[NB * NB];
    __shared__ double s_alpha[MM];
    __shared__ int s_valid[MM];
    const int lane = threadIdx.x;
    for (int k = lane; k < NB * NB; k += 64) sG[k] = gram[k];
    if (lane < MM) s_valid[lane] = lane < m ? istate[lane] : 0;
    __syncthreads();
    int dropped = 0;
    if (form) {
        const double sy = sG[newest * NB + MM + newest], ss = sG[newest * NB + newest], yy = sG[(MM + newest) * NB + MM + newest];
        const bool ok = sy > AMM_MIN_CURVATURE * sqrt(ss * yy);        // (false for NaN too)
        dropped = ok ? 0 : 1;
        __syncthreads();
        if (lane == 0) {
            s_valid[newest] = ok ? 1 : 0;
            istate[newest] = ok ? 1 : 0;
            if (!ok) istate[AMM_MIN_I_DROPPED] += 1;
        }
        __syncthreads();
    }
    // lanes of the basis vectors in use (the others hold delta = 0 and stay out of every sum: their Gram entries may be stale)
    const bool in_use = lane == 2 * MM || (lane < 2 * MM && s_valid[lane & (MM - 1)] != 0);
    auto dot_row = [&](int row, double dl) {
        double v = in_use ? dl * sG[row * NB + lane] : 0.0;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        return v;
    };
    double dl = lane == 2 * MM ? -1.0 : 0.0;          // q = -g: the recursion then ends in d itself
    int nvalid = 0, first = -1;
    for (int t = 0; t < m; ++t) {                     // newest to oldest
        const int k = (newest - t + 2 * m) % m;
        if (!s_valid[k]) continue;
        if (first < 0) first = k;
        ++nvalid;
        const double a = dot_row(k, dl) / sG[k * NB + MM + k];
        if (lane == 0) s_alpha[k] = a;
        if (lane == MM + k) dl -= a;
    }
    __syncthreads();
    if (first >= 0) dl *= sG[first * NB + MM + first] / sG[(MM + first) * NB + MM + first];        // gamma = s.y / y.y of the newest pair
    for (int t = m - 1; t >= 0; --t) {                // oldest to newest
        const int k = (newest - t + 2 * m) % m;
        if (!s_valid[k]) continue;
        const double b = dot_row(MM + k, dl) / sG[k * NB + MM + k];
        if (lane == k) dl += s_alpha[k] - b;
    }
    double gd = dot_row(2 * MM, dl);
    if (!(gd < 0.0)) {                                // not a descent direction (or NaN): steepest descent
        dl = lane == 2 * MM ? -1.0 : 0.0;
        gd = -sG[2 * MM * NB + 2 * MM];
        if (lane == 0 && nvalid > 0) istate[AMM_MIN_I_RESETS] += 1;
    }
    if (lane < NB) delta[lane] = dl;
    if (lane == 0) {
        scal[1] = gd;
        scal[4] = (double)dropped;
        scal[5] = (double)nvalid;
        scal[7] = 0.0;
    }
}

// d = sum_j delta_j b_j, one thread per atom; scal[7] <- max over the atoms of |d_atom|^2.  The maximum is taken on the bit patterns
// (non-negative doubles order like their bits): an integer atomic, the same result in any order.
__global__ void __launch_bounds__(256) k_min_combine(int n, int m, const double *delta, const double *ring, const double *gprev,
                                                     double *dir, double *scal) {
    constexpr int MM = AMM_MIN_MAXM;
    __shared__ double sd[AMM_MIN_NB];
    __shared__ double red[4];
    if (threadIdx.x < AMM_MIN_NB) sd[threadIdx.x] = delta[threadIdx.x];
    __syncthreads();
    const long long n3 = 3ll * n;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long t = 3ll * i + c;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < MM; ++j)
                if (j < m && sd[j] != 0.0) acc += sd[j] * ring[(long long)j * n3 + t];
#pragma unroll
            for (int j = 0; j < MM; ++j)
                if (j < m && sd[MM + j] != 0.0) acc += sd[MM + j] * ring[(long long)(m + j) * n3 + t];
            acc += sd[2 * MM] * gprev[t];
            dir[t] = acc;
            d2 += acc * acc;
        }
    }
    for (int off = 32; off > 0; off >>= 1) d2 = fmax(d2, __shfl_xor(d2, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d2;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double most = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        if (most > 0.0) atomicMax((unsigned long long *)&scal[7], (unsigned long long)__double_as_longlong(most));
    }
}

// x_out = x_prev + a d, a = alpha cut down to max_step / (largest |d_atom|); atoms of mass 0 and a = 0 copy x_prev bit for bit.
// scal[0] <- 0 (the energy of the evaluation that follows is added there), scal[6] <- a.
__global__ void __launch_bounds__(256) k_min_trial(long long n3, double alpha, double max_step, const double *xprev, const double *dir,
                                                   const double *mass, double *xout, double *scal) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const double dmax = sqrt(scal[7]);
    const double a = alpha * dmax > max_step ? max_step / dmax : alpha;
    if (t == 0) {
        scal[0] = 0.0;
        scal[6] = a;
    }
    if (t >= n3) return;
    const bool moves = a != 0.0 && (!mass || mass[t / 3] > 0.0);
    const double x0 = xprev[t];
    xout[t] = moves ? x0 + a * dir[t] : x0;
}

static MinObj *get_min(amm_ctx *ctx, int id, const char *who) {
    if (!ctx || id < 0 || id >= (int)ctx->minimizers.size() || !ctx->minimizers[id]) {
        amm_set_error(std::string(who) + ": invalid minimiser id");
        return nullptr;
    }
    return ctx->minimizers[id];
}

static int min_grid(long long n3) {
    const long long want = (n3 + 1023) / 1024;       // four elements per thread before the grid stops growing
    return (int)std::max<long long>(1, std::min<long long>(want, AMM_MIN_MAXBLOCKS));
}

int amm_min_free(MinObj *mo) {
    if (!mo) return 0;
    void *bufs[] = {mo->d_ring, mo->d_xprev, mo->d_gprev, mo->d_dir, mo->d_gram, mo->d_delta, mo->d_part, mo->d_istate, mo->d_ticket};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete mo;
    return 0;
}

int amm_min_create_impl(amm_ctx *ctx, int memory, double max_step, int force_input, const double *d_mass, double *d_scalars, int *id) {
    if (memory < 1 || memory > AMM_MIN_MAXM) {
        amm_set_error("amm_min_create: memory must be 1 .. " + std::to_string(AMM_MIN_MAXM));
        return 1;
    }
    if (!(max_step > 0.0)) max_step = 0.1;
    AMM_HIP(hipSetDevice(ctx->device));
    MinObj *mo = new MinObj();
    mo->n = ctx->n;
    mo->m = memory;
    mo->max_step = max_step;
    mo->sign = force_input ? -1.0 : 1.0;
    mo->d_mass = d_mass;
    mo->d_scal = d_scalars;
    const size_t n3 = 3 * (size_t)ctx->n;
    auto fail = [&]() {
        amm_min_free(mo);
        return 1;
    };
#define MIN_ALLOC(ptr, bytes)                                                                     \
    do {                                                                                          \
        hipError_t e_ = hipMalloc(&(ptr), (bytes));                                               \
        if (e_ == hipSuccess) e_ = hipMemsetAsync((ptr), 0, (bytes), ctx->stream);                \
        if (e_ != hipSuccess) {                                                                   \
            amm_set_error(std::string("amm_min_create: ") + hipGetErrorString(e_));               \
            return fail();                                                                        \
        }                                                                                         \
    } while (0)
    MIN_ALLOC(mo->d_ring, sizeof(double) * 2 * memory * n3);
    MIN_ALLOC(mo->d_xprev, sizeof(double) * n3);
    MIN_ALLOC(mo->d_gprev, sizeof(double) * n3);
    MIN_ALLOC(mo->d_dir, sizeof(double) * n3);
    MIN_ALLOC(mo->d_gram, sizeof(double) * AMM_MIN_NB * AMM_MIN_NB);
    MIN_ALLOC(mo->d_delta, sizeof(double) * AMM_MIN_NVP);
    MIN_ALLOC(mo->d_part, sizeof(double) * AMM_MIN_MAXBLOCKS * AMM_MIN_NVP);
    MIN_ALLOC(mo->d_istate, sizeof(int) * AMM_MIN_ISTATE);
    MIN_ALLOC(mo->d_ticket, sizeof(int) * AMM_TICKET_INTS);
#undef MIN_ALLOC
    if (hipMemsetAsync(d_scalars, 0, 8 * sizeof(double), ctx->stream) != hipSuccess) {
        amm_set_error("amm_min_create: the scalar block is not device memory");
        return fail();
    }
    ctx->minimizers.push_back(mo);
    *id = (int)ctx->minimizers.size() - 1;
    return 0;
}

int amm_min_release_impl(amm_ctx *ctx, int id) {
    MinObj *mo = get_min(ctx, id, "amm_min_release");
    if (!mo) return 1;
    AMM_HIP(hipStreamSynchronize(ctx->stream));        // nothing in flight may still read it
    amm_min_free(mo);
    ctx->minimizers[id] = nullptr;                     // (the id stays retired)
    return 0;
}

static int min_direction(amm_ctx *ctx, MinObj *mo, int newest, int form) {
    hipLaunchKernelGGL(k_min_coef, dim3(1), dim3(64), 0, ctx->stream, mo->m, newest, form, mo->d_gram, mo->d_delta, mo->d_scal,
                       mo->d_istate);
    hipLaunchKernelGGL(k_min_combine, dim3((mo->n + 255) / 256), dim3(256), 0, ctx->stream, mo->n, mo->m, mo->d_delta, mo->d_ring,
                       mo->d_gprev, mo->d_dir, mo->d_scal);
    AMM_HIP(hipGetLastError());
    return 0;
}

static int min_gram(amm_ctx *ctx, MinObj *mo, const double *d_x, const double *d_g, int form) {
    MinGramArgs A;
    A.n3 = 3ll * mo->n;
    A.m = mo->m;
    A.p = mo->head;
    A.form = form;
    A.sign = mo->sign;
    A.x = d_x;
    A.g = d_g;
    A.mass = mo->d_mass;
    A.ring = mo->d_ring;
    A.xprev = mo->d_xprev;
    A.gprev = mo->d_gprev;
    A.part = mo->d_part;
    A.gram = mo->d_gram;
    A.scal = mo->d_scal;
    A.ticket = mo->d_ticket;
    hipLaunchKernelGGL(k_min_gram, dim3(min_grid(A.n3)), dim3(256), 0, ctx->stream, A);
    AMM_HIP(hipGetLastError());
    return 0;
}

int amm_min_begin_impl(amm_ctx *ctx, int id, const double *d_x, const double *d_g) {
    MinObj *mo = get_min(ctx, id, "amm_min_begin");
    if (!mo) return 1;
    if ((d_x == nullptr) != (d_g == nullptr) || (!d_x && !mo->begun)) {
        amm_set_error("amm_min_begin: positions and gradient, or neither (restart from the stored ones, after a first begin)");
        return 1;
    }
    AMM_HIP(hipMemsetAsync(mo->d_istate, 0, sizeof(int) * 16, ctx->stream));      // no pair is valid
    mo->head = 0;
    if (d_x) {
        if (min_gram(ctx, mo, d_x, d_g, 0)) return 1;
        mo->begun = true;
    } else {
        mo->n_restarts++;
    }
    return min_direction(ctx, mo, 0, 0);
}

int amm_min_advance_impl(amm_ctx *ctx, int id, const double *d_x, const double *d_g) {
    MinObj *mo = get_min(ctx, id, "amm_min_advance");
    if (!mo) return 1;
    if (!d_x || !d_g || !mo->begun) {
        amm_set_error("amm_min_advance: needs positions and a gradient, after amm_min_begin");
        return 1;
    }
    const int p = mo->head;
    if (min_gram(ctx, mo, d_x, d_g, 1)) return 1;
    mo->head = (p + 1) % mo->m;
    mo->n_advances++;
    return min_direction(ctx, mo, p, 1);
}

int amm_min_trial_impl(amm_ctx *ctx, int id, double alpha, double *d_x_out) {
    MinObj *mo = get_min(ctx, id, "amm_min_trial");
    if (!mo) return 1;
    if (!d_x_out || !mo->begun || !(alpha >= 0.0)) {
        amm_set_error("amm_min_trial: needs an output buffer and alpha >= 0, after amm_min_begin");
        return 1;
    }
    const long long n3 = 3ll * mo->n;
    hipLaunchKernelGGL(k_min_trial, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, ctx->stream, n3, alpha, mo->max_step, mo->d_xprev,
                       mo->d_dir, mo->d_mass, d_x_out, mo->d_scal);
    AMM_HIP(hipGetLastError());
    mo->n_trials++;
    return 0;
}

int amm_min_scalars_impl(amm_ctx *ctx, int id, double out[8]) {
    MinObj *mo = get_min(ctx, id, "amm_min_scalars");
    if (!mo || !out) return 1;
    AMM_HIP(hipMemcpyAsync(out, mo->d_scal, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return amm_comm_wait_impl(ctx, "amm_min_scalars");
}

int amm_min_stats_impl(amm_ctx *ctx, int id, int64_t out[8]) {
    MinObj *mo = get_min(ctx, id, "amm_min_stats");
    if (!mo || !out) return 1;
    int h[AMM_MIN_ISTATE];
    AMM_HIP(hipMemcpyAsync(h, mo->d_istate, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    if (amm_comm_wait_impl(ctx, "amm_min_stats")) return 1;
    int valid = 0;
    for (int j = 0; j < mo->m; ++j) valid += h[j] != 0;
    out[0] = mo->n_advances;
    out[1] = mo->n_trials;
    out[2] = h[AMM_MIN_I_DROPPED];
    out[3] = mo->n_restarts;
    out[4] = h[AMM_MIN_I_RESETS];
    out[5] = valid;
    out[6] = mo->m;
    out[7] = 0;
    return 0;
}

// what 0: the Gram matrix, (2m+1)^2 doubles in the order [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g]; 1: delta, 2m+1; 2: d, 3n.
int amm_min_read_impl(amm_ctx *ctx, int id, int what, double *h_out) {
    MinObj *mo = get_min(ctx, id, "amm_min_read");
    if (!mo || !h_out) return 1;
    constexpr int MM = AMM_MIN_MAXM, NB = AMM_MIN_NB;
    const int m = mo->m, nb = 2 * m + 1;
    auto wide = [&](int j) { return j < m ? j : (j < 2 * m ? MM + (j - m) : 2 * MM); };
    if (amm_comm_wait_impl(ctx, "amm_min_read")) return 1;
    if (what == 0) {
        double g[NB * NB];
        AMM_HIP(hipMemcpy(g, mo->d_gram, sizeof(g), hipMemcpyDeviceToHost));
        for (int a = 0; a < nb; ++a)
            for (int b = 0; b < nb; ++b) h_out[a * nb + b] = g[wide(a) * NB + wide(b)];
    } else if (what == 1) {
        double d[NB];
        AMM_HIP(hipMemcpy(d, mo->d_delta, sizeof(d), hipMemcpyDeviceToHost));
        for (int a = 0; a < nb; ++a) h_out[a] = d[wide(a)];
    } else if (what == 2) {
        AMM_HIP(hipMemcpy(h_out, mo->d_dir, sizeof(double) * 3 * (size_t)mo->n, hipMemcpyDeviceToHost));
    } else {
        amm_set_error("amm_min_read: what = 0 (Gram matrix), 1 (delta) or 2 (direction)");
        return 1;
    }
    return 0;
}
