/*
 * include/atomsmm_hip.h -- C-ABI of libatomsmm_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of AtomsMM: the RESPA-split nonbonded pair forces and the
 * multiple-timescale propagator inner loop.  AtomsMM has no FFI of its own: it subclasses OpenMM's
 * SWIG classes and OpenMM's C++ does the arithmetic.  Each entry point below
 * therefore names the OpenMM call *as made by the reference* (file:line in /root/reference) whose
 * work it takes over.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - return 0 = OK; non-zero = error, message via amm_last_error().
 *   - `h_` pointers are HOST memory (copied during the call, caller keeps ownership);
 *     `d_` pointers are DEVICE memory owned by the caller (e.g. torch tensors), fp64, C-contiguous;
 *     per-atom vectors are AoS [n_atoms][3].
 *   - units: nm, ps, dalton, kJ/mol, elementary charge (OpenMM's unit system).
 *   - all work is enqueued on the context's HIP stream; nothing synchronises unless stated.
 *   - one context per process per GPU; not thread-safe.
 *   - atom decomposition: amm_set_slice(rank, world) makes pair forces compute only the rows of this
 *     rank's slice of the cell-sorted order (owner-computes: every force row has one producer).  The
 *     default exchange of a group that holds one pair force is an ALL-GATHER of those slices
 *     (AMM_EXCHANGE_GATHER: each rank leaves its rows, in sorted order, in its chunk of the exchange
 *     buffer; 1/world of the bytes of an all-reduce and no additions); groups that also hold sliced
 *     bond lists or reciprocal space, and hybrid lists, write zeros for the rows they do not own and
 *     all-reduce(sum) the buffer (AMM_OP_ALLREDUCE).  Either is issued by the library itself on its
 *     own RCCL communicator (amm_comm_init), which keeps a whole multi-rank step program inside one
 *     amm_run_ops call, or by the host (torch.distributed) between amm_run_ops calls.
 */
#ifndef ATOMSMM_HIP_H
#define ATOMSMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMM_ABI_VERSION 1

/* ---- pair-energy families -------------------------------------------------------------------- */
enum {
    AMM_NEAR_NONE = 0,      /* S(u) V_LJC                      NearForce._expressions forces.py:541-543 */
    AMM_NEAR_SHIFT = 1,     /* S(u) (V_LJC(r) - V_LJC(rc0))    forces.py:544-548                        */
    AMM_NEAR_FSWITCH = 2,   /* force-switched LJC              forces.py:549-563 (V' = S V'_LJC, :628)  */
    AMM_DAMPED = 3,         /* DampedSmoothedForce             forces.py:448-455                        */
    AMM_NONBONDED = 4,      /* _AtomsMM_NonbondedForce direct space  forces.py:134-190, 723             */
    AMM_SOFTCORE = 5,       /* SolvationSystem's solute-solvent softcore LJ, 4 lambda eps (1-x)/x^2 with
                               x = (r/sigma)^6 + (1-lambda)/2, restricted to an interaction group
                               (systems.py:266-272).  lambda = desc.alpha; the charge array carries the set of
                               each atom (1, 2, 0 = neither; use Kc = 1): a pair counts iff the codes multiply
                               to 2; AMM_SWITCH = OpenMM's built-in switch imported with the cutoff            */
    AMM_LJ_VIRIAL = 6,      /* ComputingSystem's dispersion virial as an energy, 24 eps (2 (sigma/r)^12 - (sigma/r)^6)
                               (systems.py:894), AMM_SWITCH as imported                                        */
    AMM_PAIR_EXPR = 7       /* any other energy text of a CustomNonbondedForce, compiled by the host and interpreted per
                               pair together with its derivative in r (csrc/pair_expr.hip); created by
                               amm_pair_expr_create only.  AMM_SWITCH = OpenMM's built-in switch rswitch -> rc      */
};
enum {
    AMM_GUARD_RC0 = 1,      /* energy *= step(rc0 - r)         forces.py:661, 714 ; systems.py:73      */
    AMM_COULOMB_EWALD = 2,  /* NONBONDED: Kc qq erfc(alpha r)/r                                         */
    AMM_COULOMB_RF = 4,     /* NONBONDED: reaction field (parity unpinned)              */
    AMM_SWITCH = 8,         /* NONBONDED / SOFTCORE: OpenMM built-in switch rswitch -> rc                */
    AMM_NO_SHIFT = 16,      /* NEAR_FSWITCH: energy without the constant -V*(rc0) (AlchemicalRespaSystem's
                               force-switched potentials, systems.py:823-846)                            */
    AMM_GROUP_LJ = 32,      /* interaction group for Lennard-Jones-only forces: the charge array carries the set
                               of each atom (1, 2, 0; Kc = 1), a pair counts iff the codes multiply to 2, no
                               Coulomb term (systems.py:739-772)                                         */
    AMM_GROUP_Q = 64,       /* interaction group for Coulomb-only forces (the force-switched solute-solvent
                               electrostatics of Coulomb scaling, systems.py:696-708, 848-856): the sigma array
                               carries TWICE the set code of each atom (2, 4, 0): the mixed sigma (sigma_i +
                               sigma_j)/2 = 3 selects a (set 1, set 2) pair; epsilon is ignored         */
    AMM_FREE_SPACE = 128    /* nonbondedMethod NoCutoff / CutoffNonPeriodic (forces.py:278-283; systems.py:371-372,
                               850-851): every pair that is not excluded, at the distance the positions give -- no box,
                               no minimum image, no neighbour list (csrc/free.hip walks all n^2 pairs; at most 32768
                               atoms).  rc > 0: pairs with r >= rc skipped (CutoffNonPeriodic); rc <= 0: no cutoff
                               (NONBONDED only: no switch and no reaction-field term are applied).  Families NEAR_*,
                               DAMPED and NONBONDED with plain or reaction-field Coulomb; no interaction groups.
                               amm_pair_set_params and amm_pair_set_scale work on such a force; amm_pair_share_list,
                               amm_pair_set_lambda[_dev], amm_pair_energy_derivative, amm_pair_energy_states and
                               amm_pair_count_within return non-zero; amm_pair_get_stats reports its evaluations, zero
                               builds and list_kind 4.  Single rank only.                                */
};

typedef struct {
    int32_t family;
    int32_t flags;
    int32_t degree;   /* DAMPED: u = (r^d - rs^d)/(rc^d - rs^d); d = 1 is OpenMM's built-in switch */
    int32_t pad_;
    double sign;      /* +1 / -1 (subtract=True forces.py:662; discount forces.py:714)            */
    double rc;        /* cutoff actually used: pairs with r >= rc skipped                          */
    double rswitch;   /* DAMPED / NONBONDED switch start                                           */
    double rc0, rs0;  /* near-force cutoff / switch start                                          */
    double alpha;     /* erfc damping, 1/nm                                                        */
    double Kc;        /* 138.935456  forces.py:407                                                 */
    double krf, crf;  /* reaction field constants                                                  */
} amm_pair_desc;

/* ---- bonded term kinds (owner-computes, no atomics) ------------------------------------------ */
enum {
    AMM_BOND_HARMONIC = 0,   /* idx[2], params (r0, k)            OpenMM HarmonicBondForce (group 0)       */
    AMM_ANGLE_HARMONIC = 1,  /* idx[3], params (theta0, k)        OpenMM HarmonicAngleForce                */
    AMM_BOND_LJC = 2,        /* idx[2], params (qq, sigma, eps)   NonbondedExceptionsForce forces.py:400-407 */
    AMM_BOND_NEAR = 3,       /* idx[2], params (qq, sigma, eps)   NearExceptionForce forces.py:673-680     */
    AMM_TORSION_PERIODIC = 4,/* idx[4], params (n, phase, k)      OpenMM PeriodicTorsionForce              */
    AMM_BOND_EWALD_EXCL = 5, /* idx[2], params (qi*qj)            -Kc qi qj erf(alpha r)/r, NonbondedForce exclusion term */
    AMM_BOND_VIRIAL_HARMONIC = 6, /* idx[2], params (r0, k)       -k r (r - r0): bond-stretching virial, ComputingSystem systems.py:914 */
    AMM_BOND_VIRIAL_LJ = 7   /* idx[2], params (qq, sigma, eps)   24 eps (2 x^2 - x), x = (sigma/r)^6: exception virial systems.py:898 */
};

/* ---- step-program ops (one flat, unrolled outer step; built by the host from the step program
 *      that RespaPropagator.addSteps emits, propagators.py:933-973) ------------------------------ */
enum {
    AMM_OP_EVAL = 1,   /* a = group: buffer[group_slot(a)] <- sum of the group's forces at current x */
    AMM_OP_KICK = 2,   /* v <- v + coef*(buf[a] -/+ buf[b])/m  (b = -1: single buffer; c = 1: plus)  propagators.py:271,
                          force expressions (f0), (f2-f1), (f0+fm1) ... of propagators.py:917-928 */
    AMM_OP_MOVE = 3,   /* x <- x + coef*v                                                propagators.py:249
                          (regulated mode, amm_regulated_define: x <- x + c tanh(alpha v/c) coef)         */
    AMM_OP_COPY = 4,   /* buf[a] <- buf[b]                          integrators.py:139-144 (`_f2_ <- f2`)    */
    AMM_OP_COMBINE = 5,/* buf[a] <- buf[b] + coef*buf[c]            propagators.py:951 (`fm2 <- f2-f1`)       */
    AMM_OP_EXPR = 6,   /* buf[b] <- per-DOF expression a (amm_expr_define): bath steps inside a RESPA loop, e.g. a
                          thermostat update on a per-DOF variable (NHL_R, integrators.py:272-318); each execution draws from the
                          next random-stream counter                                                                  */
    AMM_OP_BATH = 7,   /* v <- z v + sqrt(kT (1 - z^2)/m) gaussian with (z, kT) = bath a (amm_bath_define): the Ornstein-Uhlenbeck
                          step of OrnsteinUhlenbeckPropagator on (v, m) without force (propagators.py:727-741), as a native op so
                          that the inner-loop kernel can carry it (Langevin_R 'middle' scheme)                        */
    AMM_OP_SAVE_REF = 8,    /* reference positions of the constraint solver <- x (start of a step)                   */
    AMM_OP_CONSTRAIN_X = 9, /* addConstrainPositions (propagators.py:250, 1129): SHAKE along the reference bond vectors,
                               then reference <- x                                                                    */
    AMM_OP_CONSTRAIN_V = 10,/* addConstrainVelocities (propagators.py:272, 1131): RATTLE                              */
    AMM_OP_ALLREDUCE = 11,  /* buf[a] <- sum over ranks of buf[a] (RCCL, the context's own communicator: amm_comm_init):
                               the exchange of atom decomposition after the EVAL of a sliced group      */
    AMM_OP_STOCK = 12,      /* the whole post-force update of one step of stock integrator a (amm_stock_define) with the forces
                               in buf[b], in ONE launch: kick, RATTLE, moves, bath, SHAKE and velocity correction per constraint
                               cluster (or per atom of no cluster); takes one random-stream counter                     */
    AMM_OP_DRUDE_STEP = 13  /* the whole post-force update of one step of Drude step a (amm_drude_step_define) with the forces in
                               buf[b], in ONE launch: the dual Langevin thermostat of every Drude pair and the Langevin step of
                               every other atom, SHAKE, the hard wall; takes one random-stream counter                  */
};
typedef struct {
    int32_t op, a, b, c;
    double coef;
} amm_op;

typedef struct amm_ctx amm_ctx;

int amm_abi_version(void);
const char *amm_last_error(void);

/* Context.__init__ / Context.setPeriodicBoxVectors  (utils.py:153-155 builds the Simulation/Context).
 * stream: hipStream_t as void* (NULL = default stream).
 * h_box = NULL: a context without a periodic box (a System without box vectors: a solute in vacuum, a droplet).  It holds
 * free-space pair forces (AMM_FREE_SPACE) and bond-list terms with periodic = 0; amm_pair_create without that flag, bond-list
 * terms with periodic != 0, amm_pme_create, amm_set_box and amm_mol_scale return non-zero with "the context has no periodic
 * box" on it.  A context created with a box accepts free-space forces too. */
int amm_create(int32_t n_atoms, const double h_box[3], int32_t device, void *stream, amm_ctx **out);
int amm_destroy(amm_ctx *ctx);
int amm_set_stream(amm_ctx *ctx, void *stream);
int amm_set_slice(amm_ctx *ctx, int32_t rank, int32_t world);
/* The library's own RCCL communicator (one rank per process per GPU).  Rank 0 makes an id (amm_comm_unique_id), the
 * host distributes its 128 bytes to all ranks by any means (torch.distributed broadcast, MPI, a file) and every rank
 * calls amm_comm_init (collective, blocks until all ranks joined).  rccl_path: the librccl to bind (a torch process
 * passes torch/lib/librccl.so so that one copy serves both), NULL = the dynamic loader's default.
 * No reference counterpart: AtomsMM/OpenMM are single-device. */
#define AMM_COMM_ID_BYTES 128
int amm_comm_unique_id(const char *rccl_path, uint8_t id[AMM_COMM_ID_BYTES]);
int amm_comm_init(amm_ctx *ctx, const char *rccl_path, const uint8_t id[AMM_COMM_ID_BYTES], int32_t rank, int32_t world);
/* releases the communicator (amm_destroy does it too); collective, like ncclCommDestroy.  Errors of the communicator: an enqueue that
 * fails returns non-zero at once; an ASYNCHRONOUS error (a peer rank died, a link failed: ncclCommGetAsyncError) is polled after every
 * collective the library enqueues and by amm_check / amm_synchronize / amm_comm_destroy, whose waits for the stream are bounded by the
 * option "comm_timeout" -- in either case the communicator is aborted (ncclCommAbort), the call returns non-zero with the reason in
 * amm_last_error, and every later collective of the context fails the same way (failure detection). */
int amm_comm_destroy(amm_ctx *ctx);
/* in-place sum over ranks of count doubles in device memory, on the context's stream */
int amm_comm_allreduce(amm_ctx *ctx, double *d_buf, int64_t count);
/* Exchange of owner-computed force slices by ALL-GATHER instead of all-reduce (1/world of the bytes, no additions).
 * A group in AMM_EXCHANGE_GATHER mode must hold exactly one pair force.  Its EVAL op leaves the rows of the rank's slice
 * of the cell-sorted order in chunk `rank` of the exchange buffer (caller-owned, world x 2 x ceil(n/world) x 3 doubles;
 * a dual evaluation fills [2][ceil(n/world)][3] per chunk, a single one [ceil(n/world)][3]), all-gathers the chunks on
 * the library's communicator and spreads them to the group's buffer in atom order (every rank holds the same
 * permutation).  Without a communicator the EVAL must be the last op of its amm_run_ops call: the host gathers the
 * chunks (count per rank = forces x ceil(n/world) x 3 doubles) and calls amm_exchange_finish. */
enum { AMM_EXCHANGE_REDUCE = 0, AMM_EXCHANGE_GATHER = 1 };
int amm_group_set_exchange(amm_ctx *ctx, int32_t group, int32_t mode);
int amm_bind_exchange(amm_ctx *ctx, double *d_buf, int64_t n_doubles);
int amm_exchange_finish(amm_ctx *ctx);
/* *nf = 0: no exchange is waiting; else every rank's chunk of the exchange buffer holds nf x amm_exchange_per() x 3 doubles to all-gather
 * (1: one force; 2: the two forces of a dual evaluation, or positions + velocities of a state exchange -- see amm_run_stats) */
int amm_exchange_pending(amm_ctx *ctx, int32_t *nf);
/* out[0] = collectives issued so far, out[1] = doubles per rank they carried (AMM_OP_ALLREDUCE ops on buffers that are
 * neighbours in memory are merged into one message) */
int amm_comm_stats(amm_ctx *ctx, int64_t out[2]);
int amm_synchronize(amm_ctx *ctx);
/* Raises pending device-side errors (neighbour-list overflow, NaN guard): returns non-zero + message. Synchronises.
 * A constraint cluster that the solvers left unconverged is one of them, and a cluster whose positions or velocities are not finite
 * (NaN or infinite, on entry or by a blow-up of the sweep) counts as unconverged; the flag is cleared by the call that reports it. */
int amm_check(amm_ctx *ctx);

/* CustomNonbondedForce(energy) + addParticle + addExclusion  (forces.py:225, 299-312; systems.py:97-111).
 * h_excl: E pairs (i,j) -- every exception of the source NonbondedForce becomes an exclusion.
 * skin: Verlet buffer (nm) for the cell-list-built neighbour list; <0 = default. */
int amm_pair_create(amm_ctx *ctx, const amm_pair_desc *desc, const double *h_q, const double *h_sigma,
                    const double *h_eps, const int32_t *h_excl, int32_t n_excl, double skin,
                    int32_t *force_id);
/* setParticleParameters + updateParametersInContext / Context.setParameter for offset parameters
 * (forces.py:247-258, 292-309: charge+lambda*chargeScale ...). Effective values are passed. */
int amm_pair_set_params(amm_ctx *ctx, int32_t force_id, const double *h_q, const double *h_sigma,
                        const double *h_eps);
/* CustomNonbondedForce(energy) with ANY energy text + addPerParticleParameter / addGlobalParameter + addParticle + addExclusion,
 * CutoffPeriodic (what OpenMM compiles with Lepton; the reference's forces are the texts amm_pair_create knows by family).
 * desc->family = AMM_PAIR_EXPR; only rc, rswitch, flags & AMM_SWITCH and sign are read (AMM_FREE_SPACE: non-zero).  code / consts /
 * globals: the program of atomsmm_amd.expr.compile_pair -- postfix words opcode | arg << 8 over r (opcode 50), the row atom's
 * parameters <name>1 (51, arg = slot), the neighbour's <name>2 (52), constants (0), globals (1), locals (6 / 7) and the arithmetic
 * and function opcodes of csrc/expr_vm.h; at most 256 words, 48 constants, 48 globals, stack depth 16, 16 locals (csrc/pair_expr_vm.h),
 * checked here.  h_p0..h_p2: the three per-particle parameter slots, stored RAW (NULL = all zero).  Each pair is evaluated from both
 * rows and counted once, so the text must be symmetric under 1 <-> 2.  The force is an ordinary member of a group and walks per-atom
 * rows (list_kind 0) of its own: amm_pair_share_list, amm_pair_set_lambda[_dev], amm_pair_energy_derivative, amm_pair_energy_states
 * and amm_pair_create with this family return non-zero with a message naming the family; amm_pair_set_params stores raw values;
 * amm_pair_get_stats, amm_pair_count_within, amm_set_box and the profile hooks work as for any per-atom-row force. */
int amm_pair_expr_create(amm_ctx *ctx, const amm_pair_desc *desc, const int32_t *code, int32_t ncode, const double *consts,
                         int32_t nconst, const double *globals, int32_t nglobal, const double *h_p0, const double *h_p1,
                         const double *h_p2, const int32_t *h_excl, int32_t n_excl, double skin, int32_t *force_id);
/* Context.setParameter(name, value) for a global parameter of such a force: all of the program's globals, in its order. */
int amm_pair_expr_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* addTabulatedFunction on such a force: the tables that the words 55 (Continuous1DFunction), 56 (Discrete1DFunction) and 57
 * (Discrete2DFunction) of its program read -- a word's arg is the index of its table here, the force's function order; compile_pair
 * emits it behind the word's arguments.  Table k: */
enum {
    AMM_TABLE_CONTINUOUS1D = 0, /* dims[2k] = knots (>= 2), equally spaced on ranges[2k] < ranges[2k+1]; its doubles: 4 per interval,
                                   (a, b, c, d) of a + u (b + u (c + u d)), u = t - the interval's left knot -- the natural cubic
                                   spline solved by the host (atomsmm_amd/tables.py).  Outside the range: value and derivative 0   */
    AMM_TABLE_DISCRETE1D = 1,   /* dims[2k] = values; values[rint(t)], derivative 0                                                 */
    AMM_TABLE_DISCRETE2D = 2    /* dims[2k] x dims[2k+1] values, values[rint(x) + dims[2k] * rint(y)] (OpenMM's layout), derivative 0 */
};
/* kinds[n_tables], dims[2 n_tables], ranges[2 n_tables] (read for a continuous table only), offsets[n_tables]: where table k's
 * doubles begin in data[n_data]; 0 <= n_tables <= 8.  Non-zero with a message naming the word when a table word of the program has
 * no table (arg >= n_tables) or a table of another kind (and so another number of arguments), when a table does not lie inside
 * data, a continuous table has fewer than 2 knots or no finite min < max.  The tables are copied to one device allocation that the
 * force owns.  A discrete index that is NaN or outside its table gives NaN for that pair, and no index of any kind reads outside the
 * allocation.  Calling it again uploads new VALUES (updateParametersInContext), ordered after every evaluation already queued: the
 * number of tables, their kinds and their sizes must be those of the first call.  Evaluating a force whose program has table words
 * before this call returns non-zero and launches nothing; a force whose program has none needs no call. */
int amm_pair_expr_set_tables(amm_ctx *ctx, int32_t force_id, int32_t n_tables, const int32_t *kinds, const int32_t *dims,
                             const double *ranges, const int32_t *offsets, const double *data, int32_t n_data);
/* RESPASystem puts a short-ranged copy (group 1, rcutIn) and the full force (group 2) over the SAME particles and
 * exclusions (systems.py:71-77): let `force_id` traverse the front part of `host_id`'s neighbour rows instead of
 * building its own list.  Call before the first evaluation; exclusions must be identical. */
int amm_pair_share_list(amm_ctx *ctx, int32_t force_id, int32_t host_id);

/* CustomBondForce / HarmonicBondForce / HarmonicAngleForce term lists of one force group. */
/* context.setParameter('lambda_vdw', value) for a softcore pair force (systems.py:267: global parameter). */
int amm_pair_set_lambda(amm_ctx *ctx, int32_t force_id, double value);
/* The same with lambda left on the device (an AFED step moves it with amm_expr_eval_scalar): the force's kernels read *d_lambda at
 * launch time from now on; NULL, or a later amm_pair_set_lambda, returns to the host's number.  Only the list-free evaluation of a
 * softcore force with a small set (csrc/group.hip: what SolvationSystem's solute gets) supports it; others return an error. */
int amm_pair_set_lambda_dev(amm_ctx *ctx, int32_t force_id, const double *d_lambda);
/* Overall factor of a pair force (desc.sign): a global parameter that multiplies the whole energy -- `respa_switch`, or
 * the coupling function of a CustomCVForce over this force (systems.py:738-772) -- changed by setParameter. */
int amm_pair_set_scale(amm_ctx *ctx, int32_t force_id, double scale);
/* deriv(energy, lambda) of a softcore pair force (addEnergyParameterDerivative, systems.py:712-718; used by the AFED
 * kicks, integrators.py:735-737): *d_out (device) += sum over pairs of dE/dlambda at d_pos. */
int amm_pair_energy_derivative(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_out);
/* Energies of a softcore pair force at n_states values of its lambda in one pass over its pairs: d_out[k] += E(d_lambdas[k]) at d_pos.
 * Energy only (no forces are written).  The force's own lambda -- host value or amm_pair_set_lambda_dev binding -- is neither read
 * nor changed.  1 <= n_states <= AMM_MAX_STATES (64).  A force with a small set takes one launch (csrc/group.hip); one on the list
 * path takes one energy evaluation per lambda.  Multi-rank: each rank adds its block's share (sum d_out over the ranks). */
#define AMM_MAX_STATES 64
int amm_pair_energy_states(amm_ctx *ctx, int32_t force_id, const double *d_pos, const double *d_lambdas, int32_t n_states, double *d_out);

int amm_bonded_create(amm_ctx *ctx, int32_t *force_id);
/* Accuracy of AMM_ANGLE_HARMONIC: the angle is acos(cos theta) and the force divides by sqrt(1 - cos^2 theta), so the relative error of
 * the force grows like eps / sin^2 theta.  With sin theta >= 1e-2 (an angle at least 1e-2 rad = 0.6 degrees from 0 and from pi) the force
 * is as accurate as the rounding of the input coordinates allows; closer to linearity it is finite but loses digits (1e-3 rad: about
 * 1e-10 relative; an angle within 6e-8 rad of 0 or pi is taken as exactly 0 or pi), while the energy stays good to
 * k |theta - theta0| min(8 eps / sin theta, 6e-8).  theta0 = pi itself is harmless (the force vanishes with the distance from pi). */
int amm_bonded_add_terms(amm_ctx *ctx, int32_t force_id, int32_t kind, const int32_t *h_idx,
                         const double *h_params, int32_t n_terms, int32_t periodic,
                         const amm_pair_desc *desc_or_null);
int amm_bonded_finalize(amm_ctx *ctx, int32_t force_id);
/* world > 1: evaluate only this rank's block of atoms (use for bonded sets living in an all-reduced group). */
int amm_bonded_set_sliced(amm_ctx *ctx, int32_t force_id, int32_t on);
/* Free a bond-list set the host has replaced: Context.setParameter on a parameter offset rebuilds the exception terms of the
 * NonbondedForce (forces.py:292-309, systems.py:303-311), which OpenMM does in place.  The id is retired (never reused) and
 * leaves every group definition. */
int amm_bonded_release(amm_ctx *ctx, int32_t force_id);
/* Which device layouts amm_bonded_finalize built for the set, and so which launches it admits (read-only, no device work):
 * out[0] connected components of the term graph (an atom in no term is a component of its own), out[1] atoms of the largest,
 * out[2] 1 when every component has at most G terms and the inner-components launch runs with term lanes, out[3] G (4 or 8: lanes
 * per component of that launch; rule 2 of amm_run_ops takes it when out[1] <= 8), out[4] 1 when the set is a box of three-site
 * molecules that a molecule-row pair launch can integrate as its epilogue, out[5] 1 when the fused EVAL + kicks launch runs the
 * small components four lanes each (mixed sets), out[6] terms of the term-parallel tables (0: below option terms_from, the
 * record walk is the only evaluation), out[7] small components of a mixed set.  Refused before amm_bonded_finalize. */
int amm_bonded_stats(amm_ctx *ctx, int32_t force_id, int64_t *out);

/* CustomBondForce / CustomAngleForce / CustomTorsionForce / CustomExternalForce with ANY energy text (what OpenMM compiles with
 * Lepton; the texts the reference ships are the kinds of amm_bonded_add_terms).  A force object of its own, an ordinary member of a
 * group, evaluated through amm_force_eval; the amm_bonded_* calls refuse its id.  kind: what the text's variable is -- */
typedef enum {
    AMM_TERM_BOND = 0,       /* idx[2]: r = |x0 - x1|                                               */
    AMM_TERM_ANGLE = 1,      /* idx[3]: theta in [0, pi] at atom 1 (the angle of AMM_ANGLE_HARMONIC)    */
    AMM_TERM_TORSION = 2,    /* idx[4]: theta in (-pi, pi], the dihedral of AMM_TORSION_PERIODIC         */
    AMM_TERM_EXTERNAL = 3    /* idx[1]: x, y, z of the atom as the positions give them (never wrapped)   */
} amm_term_kind;
#define AMM_TERM_MAX_PARAMS 8
/* code / consts / globals: the program of atomsmm_amd.expr.compile_term -- the words of amm_pair_expr_create, but for its leaves:
 * the term's variable k (opcode 53: r or theta is k = 0; x, y, z are k = 0, 1, 2) and the term's parameter k (54) instead of 50..52;
 * the same limits (csrc/pair_expr_vm.h), checked here with a walk of the stack.  h_idx: n_terms x 4 atom indices, padded with -1
 * behind the kind's arity; an index outside [0, n) is refused.  h_params: n_params x n_terms doubles, PARAMETER-major (all terms'
 * parameter 0, then parameter 1 ...), n_params <= AMM_TERM_MAX_PARAMS; NULL when n_params = 0.  periodic: differences of positions
 * take the minimum image (needs a context with a box; not for AMM_TERM_EXTERNAL).  Evaluation is deterministic: every term once
 * (dE/dvariable comes with E from one forward-mode pass; an external term takes three), its forces parked per role, every atom then
 * adds its records in term order; with accumulate = 0 every row of the buffer is written.  The forces of an evaluation with and
 * without energy are the same numbers. */
int amm_term_expr_create(amm_ctx *ctx, int32_t kind, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst,
                         const double *globals, int32_t nglobal, const int32_t *h_idx, const double *h_params, int32_t n_terms,
                         int32_t n_params, int32_t periodic, int32_t *force_id);
/* Context.setParameter(name, value) for a global parameter of such a force: all of the program's globals, in its order. */
int amm_term_expr_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* set*Parameters + updateParametersInContext: all per-term values again, laid out as at creation (same n_terms, n_params; the
 * atoms of a term do not change). */
int amm_term_expr_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_terms, int32_t n_params);
/* Free such a force; as amm_bonded_release, the id is retired and leaves every group definition. */
int amm_term_expr_release(amm_ctx *ctx, int32_t force_id);

/* CustomCVForce(any energy text) over several collective variables (force type AMM_FORCE_CV): E = f(cv_1 .. cv_K; globals), cv_k the
 * potential energy of inner force k at the current positions; the atoms get -sum_k df/dcv_k grad cv_k.  An ordinary member of a
 * group, evaluated through amm_force_eval; the amm_pair_*, amm_bonded_*, amm_term_expr_* and amm_pme_* calls refuse its id naming
 * AMM_FORCE_CV.  The inner forces are evaluated on the stream, then ONE launch evaluates f and its partial derivatives (one lane
 * per variable of a forward-mode pass) and combines the inner forces in the order k = 0 .. K-1: no atomics, the same bits run to run,
 * no host round trip. */
#define AMM_CV_MAX_CVS 16
#define AMM_CV_MAX_DERIVS 16
/* CustomCVForce(energy) + addCollectiveVariable x n_cv + addEnergyParameterDerivative x n_deriv.  inner_ids: n_cv ids of bond-list
 * sets (amm_bonded_create .. amm_bonded_finalize), term-expression forces (amm_term_expr_create), compound-bond forces
 * (amm_compound_create) or RMSD forces (amm_rmsd_create) that the caller created, keeps in no group and releases itself; any other type is refused.  code / consts / globals: the program of atomsmm_amd.expr.compile_cv --
 * the words of amm_term_expr_create with variable k (opcode 53) = collective variable k for k < n_cv and derivative parameter
 * k - n_cv behind them, no per-term parameters; the same limits, checked here with a walk of the stack.  Scratch: 24 n_cv n bytes. */
int amm_cv_create(amm_ctx *ctx, const int32_t *inner_ids, int32_t n_cv, int32_t n_deriv, const int32_t *code, int32_t ncode,
                  const double *consts, int32_t nconst, const double *globals, int32_t nglobal, int32_t *force_id);
/* Context.setParameter(name, value) for a global parameter of the outer text that is no derivative parameter: all of the program's
 * globals, in its order. */
int amm_cv_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* Context.setParameter(name, value) for a parameter named by addEnergyParameterDerivative: the current values of all n_deriv. */
int amm_cv_set_variables(amm_ctx *ctx, int32_t force_id, const double *values, int32_t n_deriv);
/* CustomCVForce.getCollectiveVariableValues(context): evaluates the inner forces at d_pos and copies their n_cv energies to h_out.
 * The one call of this family that waits for the stream. */
int amm_cv_values(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out);
/* State.getEnergyParameterDerivatives() / deriv(energy, p) of a CustomIntegrator: df/dp of the n_deriv derivative parameters at
 * d_pos -- the explicit dependence of the outer text -- ADDED to d_out[0 .. n_deriv) (device memory) on the stream; no wait, the
 * shape of amm_pair_energy_derivative. */
int amm_cv_energy_derivative(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_out);
/* Free such a force and its scratch; the id is retired and leaves every group definition.  The inner ids stay the caller's. */
int amm_cv_release(amm_ctx *ctx, int32_t force_id);

/* CustomCompoundBondForce / CustomCentroidBondForce(any energy text) (force type AMM_FORCE_COMPOUND): a bond is n_slots particles --
 * or, with groups, n_slots weighted centres of groups of atoms -- and its text reads up to AMM_COMPOUND_MAX_VARS geometric
 * variables over them.  An ordinary member of a group, evaluated through amm_force_eval, and a legal inner force of amm_cv_create;
 * the amm_pair_*, amm_bonded_*, amm_term_expr_* and amm_pme_* calls refuse its id naming AMM_FORCE_COMPOUND.  One lane per (bond,
 * variable) computes the variable and its gradient, then dE/dvariable by a forward-mode pass seeded in it; forces are parked per
 * (bond, variable, role) and every atom adds its records in that order: no atomics, the same bits run to run, and the forces of an
 * evaluation with and without energy are the same numbers. */
typedef enum {
    AMM_CVAR_X = 0,          /* slots[1]: raw x of the particle (never wrapped); AMM_CVAR_Y, AMM_CVAR_Z likewise */
    AMM_CVAR_Y = 1,
    AMM_CVAR_Z = 2,
    AMM_CVAR_DISTANCE = 3,   /* slots[2]: |x_a - x_b|                                                              */
    AMM_CVAR_ANGLE = 4,      /* slots[3]: the angle at the second slot, in [0, pi] (AMM_TERM_ANGLE's)              */
    AMM_CVAR_DIHEDRAL = 5    /* slots[4]: the dihedral in (-pi, pi] (AMM_TERM_TORSION's)                           */
} amm_compound_var;
#define AMM_COMPOUND_MAX_SLOTS 8
#define AMM_COMPOUND_MAX_VARS 16
/* code / consts / globals: the program of atomsmm_amd.expr.compile_compound -- the words of amm_term_expr_create with variable k
 * (opcode 53) = entry k of the variable table and parameter k (54) the bond's parameter k; the same limits, checked here with a walk
 * of the stack.  var_kinds: n_vars amm_compound_var; var_slots: n_vars x 4 positions within the bond, read up to the kind's arity;
 * a position outside [0, n_slots) is refused.  h_idx: n_bonds x n_slots atom indices (group indices with groups); an index outside
 * [0, n) (outside [0, n_groups)) is refused.  h_params: n_params x n_bonds doubles, PARAMETER-major, n_params <=
 * AMM_TERM_MAX_PARAMS; NULL when n_params = 0.  periodic: displacements inside distance / angle / dihedral take the minimum image
 * (needs a context with a box); raw coordinates never do.  n_groups = 0: the slots are particles and the three group arrays are
 * NULL.  n_groups > 0: group g has the members group_atoms[group_ptr[g] .. group_ptr[g + 1]) with the weights group_weights[..];
 * its centre is sum w_i x_i / sum w_i over the positions as given (a group is taken to be whole), and atom i of the group receives
 * w_i / W_g times the force on the centre.  An empty group, or weights that sum to zero, is refused. */
int amm_compound_create(amm_ctx *ctx, int32_t n_slots, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst,
                        const double *globals, int32_t nglobal, const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars,
                        const int32_t *h_idx, const double *h_params, int32_t n_bonds, int32_t n_params, int32_t periodic,
                        const int32_t *group_ptr, const int32_t *group_atoms, const double *group_weights, int32_t n_groups,
                        int32_t *force_id);
/* Context.setParameter(name, value) for a global parameter of such a force: all of the program's globals, in its order. */
int amm_compound_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* setBondParameters + updateParametersInContext: all per-bond values again, laid out as at creation (same n_bonds, n_params; the
 * particles or groups of a bond do not change). */
int amm_compound_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_bonds, int32_t n_params);
/* setGroupParameters + updateParametersInContext: all weights again, in the order of group_atoms (the members do not change). */
int amm_compound_set_weights(amm_ctx *ctx, int32_t force_id, const double *weights, int32_t n_members);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_compound_release(amm_ctx *ctx, int32_t force_id);

/* GBSAOBCForce: generalized-Born implicit solvent (OBC2: alpha 1, beta 0.8, gamma 4.85; dielectric offset 0.009 nm) with the
 * surface-area term 4 pi sa_energy (R + 0.14)^2 (R / B)^6, for free-space systems (csrc/gb.hip).  h_q,
 * h_radius (nm), h_scale: n_atoms doubles each -- addParticle(charge, radius, scale); eps_in / eps_out: solute and solvent
 * dielectric; sa_energy in kJ/mol/nm^2; rc <= 0: NoCutoff, otherwise CutoffNonPeriodic with the predicate r^2 < rc^2.  All pairs
 * of atoms take part (exclusions of other forces play no role), the diagonal is left out by index.  Refused: a radius <= 0.009, a
 * negative scale, a dielectric <= 0, more than 32768 atoms, more than one rank.  The force is a group member like any other:
 * amm_force_eval and amm_run_ops evaluate it, force-only or with energy; it is legal in a context created without a box.  Three
 * launches per evaluation (Born radii, pair sums, chain rule), no atomics: the same positions give the same bits. */
int amm_gb_create(amm_ctx *ctx, const double *h_q, const double *h_radius, const double *h_scale, double eps_in, double eps_out,
                  double sa_energy, double rc, int32_t *force_id);
/* setParticleParameters / setSolventDielectric / ... + updateParametersInContext: everything again, checked as at creation. */
int amm_gb_set_params(amm_ctx *ctx, int32_t force_id, const double *h_q, const double *h_radius, const double *h_scale, double eps_in,
                      double eps_out, double sa_energy, double rc);
/* The Born radii at d_pos (device, [n][3]) into h_out (host, n doubles): runs the first pass and waits (tests, diagnostics). */
int amm_gb_born_radii(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_gb_release(amm_ctx *ctx, int32_t force_id);

/* CMAPTorsionForce (force type AMM_FORCE_CMAP; csrc/cmap.hip): a term is two dihedrals, phi over the first
 * four of its eight atoms and psi over the last four (the dihedral of AMM_TORSION_PERIODIC, minimum image when periodic), and its
 * energy the value at (phi, psi) of one of n_maps maps over [0, 2 pi)^2, interpolated by the tensor-product periodic cubic spline.
 * h_sizes: n_maps grid sizes, each >= 2.  h_coeffs: the maps concatenated, 16 doubles per cell as atomsmm_amd.tables.cmap_coefficients
 * gives them: cell (s, t) of a map is row s + size * t, and E = sum_ij c[4 i + j] da^i db^j with da, db in [0, 1) the fractional
 * positions of phi and psi within the cell; sum size^2 * 16 doubles in all.  h_map_of_term: n_terms map indices; h_idx: n_terms x 8
 * atom indices (an atom may appear more than once in a term).  Refused: an atom index outside [0, n), a map index outside
 * [0, n_maps), a size below 2, periodic in a context without a box, several ranks.  The cell index is reduced modulo the size before
 * the read, so no position indexes past a map.  An ordinary member of a group, evaluated through amm_force_eval; the amm_pair_*,
 * amm_bonded_*, amm_term_expr_*, amm_compound_* and amm_pme_* calls and amm_cv_create refuse its id naming AMM_FORCE_CMAP.  Two
 * launches per evaluation (terms, then one lane per atom over its records in order), no atomics: the same positions give the same
 * bits, and the forces of an evaluation with and without energy are the same numbers. */
int amm_cmap_create(amm_ctx *ctx, int32_t n_maps, const int32_t *h_sizes, const double *h_coeffs, const int32_t *h_map_of_term,
                    const int32_t *h_idx, int32_t n_terms, int32_t periodic, int32_t *force_id);
/* setMapParameters / setTorsionParameters + updateParametersInContext: all coefficients and all map indices again, laid out as at
 * creation (same n_maps, sizes, n_terms; the atoms of a term do not change). */
int amm_cmap_set_params(amm_ctx *ctx, int32_t force_id, const double *h_coeffs, const int32_t *h_map_of_term, int32_t n_maps,
                        int32_t n_terms);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_cmap_release(amm_ctx *ctx, int32_t force_id);

/* CustomGBForce (force type AMM_FORCE_CUSTOM_GB; csrc/custom_gb.hip): a generalized-Born model written as
 * text, for free-space systems -- what OpenMM compiles with Lepton from addComputedValue / addEnergyTerm (HCT, OBC1, OBC2, GBn ...;
 * the hand-written OBC2 of amm_gb_create stays as it is).  n_values <= AMM_CGB_MAX_VALUES computed values and n_terms <=
 * AMM_CGB_MAX_TERMS energy terms, each of a type: */
typedef enum {
    AMM_CGB_SINGLE = 0,      /* SingleParticle: a text of the parameters and the values of one particle                      */
    AMM_CGB_PAIR = 1,        /* ParticlePair: a text of r and both particles, over the pairs that take part and are not excluded */
    AMM_CGB_PAIR_NOEXCL = 2  /* ParticlePairNoExclusions: ... over the pairs that take part                                     */
} amm_cgb_type;
#define AMM_CGB_MAX_VALUES 4
#define AMM_CGB_MAX_TERMS 8
/* A pair (i, j), i != j, takes part when rc <= 0 (NoCutoff) or r^2 < rc^2 (CutoffNonPeriodic).  Only computed value 0 may be of a
 * pair type: V0_i = sum over j of its text at (r; parameters of i as particle 1, of j as particle 2), ordered pairs, no symmetry
 * asked.  Value k of type SINGLE is its text at the parameters of i and V0_i .. V(k-1)_i.  The energy is the sum over i of the SINGLE
 * terms (parameters and all values of i) plus the sum over the unordered pairs of the pair terms (r, parameters and values of
 * both); a pair term is evaluated from both rows and counted half, so it must not change under 1 <-> 2 (the host checks).  Forces
 * are the full chain rule through the values.
 * types / code_ptr / const_ptr: n_values + n_terms entries (+ 1 for the two pointers), the values' programs first: program p is
 * code[code_ptr[p] .. code_ptr[p+1]) with constants consts[const_ptr[p] .. const_ptr[p+1]).  A program is what
 * atomsmm_amd.expr.compile_custom_gb emits: the words of amm_term_expr_create (variable 53, parameter 54) plus the table words 55 ..
 * 57 of amm_pair_expr_set_tables, over these leaves -- variable 0 = r, 1 + k = value k of particle 1 (in a SINGLE text: of the
 * particle), 5 + k = value k of particle 2; parameter k = of particle 1 (of the particle), 8 + k = of particle 2; global k = entry k
 * of `globals`, ONE list for all programs.  Each program obeys the limits of csrc/pair_expr_vm.h (walked here), and may read only
 * the leaves its place has (a value only the values before it; value 0 of a pair type only r and parameters).  h_params: n_params x
 * n_atoms doubles, PARAMETER-major, n_params <= AMM_TERM_MAX_PARAMS.  h_excl: n_excl pairs for the texts of type PAIR.
 * Refused: more than 32768 atoms, more than one rank, a pair-type value behind the first, a leaf outside its place, an exclusion
 * that names no pair.  An ordinary member of a group, evaluated through amm_force_eval and amm_run_ops, legal in a context without
 * a box; every other family's entry points refuse its id naming AMM_FORCE_CUSTOM_GB.  Up to four launches per evaluation (value 0,
 * the other values with their Jacobian, energy terms, chain rule), no atomics: the same positions give the same bits. */
int amm_custom_gb_create(amm_ctx *ctx, int32_t n_params, int32_t n_values, int32_t n_terms, const int32_t *types, const int32_t *code,
                         const int32_t *code_ptr, const double *consts, const int32_t *const_ptr, const double *globals, int32_t nglobal,
                         const double *h_params, const int32_t *h_excl, int32_t n_excl, double rc, int32_t *force_id);
/* setParticleParameters + updateParametersInContext: all per-particle values again, laid out as at creation. */
int amm_custom_gb_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_params, int32_t n_atoms);
/* Context.setParameter(name, value) for a global parameter of such a force: all of its globals, in the order of creation. */
int amm_custom_gb_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* addTabulatedFunction on such a force: the tables its programs' words 55 .. 57 read, with the arguments of
 * amm_pair_expr_set_tables; again with new values of the same kinds and sizes (updateParametersInContext).  A force whose programs
 * have such words evaluates only after this call. */
int amm_custom_gb_set_tables(amm_ctx *ctx, int32_t force_id, int32_t n_tables, const int32_t *kinds, const int32_t *dims,
                             const double *ranges, const int32_t *offsets, const double *data, int32_t n_data);
/* The computed values at d_pos (device, [n][3]) into h_out (host, n_values x n doubles, value-major): runs the value passes and
 * waits (tests, diagnostics; OpenMM has no such call). */
int amm_custom_gb_values(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *h_out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_custom_gb_release(amm_ctx *ctx, int32_t force_id);

/* CustomHbondForce(any energy text) (force type AMM_FORCE_HBOND; csrc/hbond.hip): n_donors donors (d1, d2, d3)
 * against n_acceptors acceptors (a1, a2, a3).  Every (donor, acceptor) pair that is not excluded and, with a cutoff, has
 * |x_d1 - x_a1| < rc contributes the text; the cutoff looks at that one distance only.  rc <= 0: NoCutoff; rc > 0 and periodic = 0:
 * CutoffNonPeriodic; periodic != 0: CutoffPeriodic -- the cutoff distance AND every displacement inside distance / angle / dihedral
 * take the minimum image, each on its own (needs a context with a box; the live box of amm_set_box is read at every evaluation).
 * code / consts / globals: the program of atomsmm_amd.expr.compile_hbond -- the words of amm_term_expr_create with variable k (opcode
 * 53) = entry k of the variable table and parameter k (54) = the donor's parameter k, behind the n_donor_params of them the
 * acceptor's; the same limits, checked here with a walk of the stack.  var_kinds: n_vars <= AMM_COMPOUND_MAX_VARS of
 * AMM_CVAR_DISTANCE / AMM_CVAR_ANGLE / AMM_CVAR_DIHEDRAL (raw coordinates are refused); var_slots: n_vars x 4 slots of the pair, 0 ..
 * 2 = d1 d2 d3, 3 .. 5 = a1 a2 a3, read up to the kind's arity.  h_donors / h_acceptors: n x 3 atom indices; the second and third may
 * be -1 (the slot is not there), and then no variable may name that slot.  h_donor_params: n_donor_params x n_donors doubles,
 * PARAMETER-major, h_acceptor_params likewise; n_donor_params + n_acceptor_params <= AMM_TERM_MAX_PARAMS.  h_excl: n_excl pairs
 * (donor index, acceptor index) -- indices of donors and acceptors, not of atoms.
 * Refused, each by name: more than 32768 donors or acceptors, the parameter and variable limits, an atom index or an exclusion index
 * out of range, a named slot left at -1, CutoffPeriodic without a box, a periodic cutoff above half the shortest box edge (also at
 * an evaluation, after the box has shrunk), more than one rank.  An ordinary member of a group, evaluated through amm_force_eval and
 * amm_run_ops, legal in a context without a box; every other family's entry points refuse its id naming AMM_FORCE_HBOND.
 * Three launches per evaluation: donor rows against acceptor columns (forces on the donors' atoms, the energy), acceptor rows
 * against donor columns (forces on the acceptors' atoms), and a gather, one lane per atom.  A wavefront owns a row (or one of its
 * "hbond_chunks" column chunks, amm_set_option), scans 64 columns at a time and queues the survivors in LDS; the interpreter runs
 * on full queues only.  No atomics: the same positions give the same bits, with and without energy. */
int amm_hbond_create(amm_ctx *ctx, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst, const double *globals,
                     int32_t nglobal, const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars, const int32_t *h_donors,
                     int32_t n_donors, const int32_t *h_acceptors, int32_t n_acceptors, const double *h_donor_params,
                     int32_t n_donor_params, const double *h_acceptor_params, int32_t n_acceptor_params, const int32_t *h_excl,
                     int32_t n_excl, double rc, int32_t periodic, int32_t *force_id);
/* setDonorParameters / setAcceptorParameters + updateParametersInContext: all per-donor and per-acceptor values again, laid out as
 * at creation (the same counts; the particles do not change). */
int amm_hbond_set_params(amm_ctx *ctx, int32_t force_id, const double *h_donor_params, int32_t n_donors, int32_t n_donor_params,
                         const double *h_acceptor_params, int32_t n_acceptors, int32_t n_acceptor_params);
/* Context.setParameter(name, value) for a global parameter of such a force: all of the program's globals, in its order. */
int amm_hbond_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* Waits for the stream.  out[0]: the ordered pairs one pass scans (n_donors x n_acceptors); out[1]: the pairs that passed the cutoff
 * and the exclusions in the last evaluation (0 before the first); out[2]: kernel launches so far; out[3]: column chunks per donor
 * row. */
int amm_hbond_stats(amm_ctx *ctx, int32_t force_id, int64_t *out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_hbond_release(amm_ctx *ctx, int32_t force_id);

/* CustomManyParticleForce(3, any energy text) (force type AMM_FORCE_MANY_PARTICLE; csrc/manyparticle.hip):
 * every set of three distinct particles {i, j, k} no pair of which is excluded contributes the text.  n_particles is 0 or the
 * context's atom count: particle i is atom i.  rc <= 0: NoCutoff (at most 2048 particles: the neighbour table is n x (n - 1));
 * rc > 0 and periodic = 0: CutoffNonPeriodic; periodic != 0: CutoffPeriodic -- the cutoff test AND every displacement inside a
 * variable take the minimum image, each on its own (needs a context with a box; the live box of amm_set_box is read at every
 * evaluation).  central = 0: SinglePermutation -- a set counts when all three distances are inside the cutoff and is evaluated once;
 * central != 0: UniqueCentralParticle -- a set counts for the centre c when the two distances from c are inside the cutoff (the
 * distance between the satellites is not tested) and is evaluated once for every such centre, which plays p1.
 * code / consts / globals: the program of atomsmm_amd.expr.compile_many_particle -- the words of amm_term_expr_create with variable k
 * (opcode 53) = entry k of the variable table and parameter k (54) = per-particle parameter k % n_params of the particle in role
 * k / n_params.  var_kinds: n_vars <= AMM_COMPOUND_MAX_VARS of AMM_CVAR_*; var_slots: n_vars x 4 slots 0 .. 2 = p1 p2 p3, read up
 * to the kind's arity.  h_params: n_params x n_particles doubles, PARAMETER-major, n_params <= 2.  h_types: the dense type index of
 * every particle, 0 .. n_types - 1, n_types <= 16.  h_perm: n_types^3 entries [t1][t2][t3] over the types of the set's tuple -- its
 * particles in ascending order, or the centre first and the satellites ascending -- each the code of the permutation of the tuple
 * that is evaluated (0 .. 5: the permutations of (0, 1, 2) in lexicographic order, role r played by element perm[r]; central mode
 * keeps the centre at p1: 0 or 1) or -1: the set is skipped.  h_excl: n_excl pairs of particles.
 * Refused, each by name: more than 32768 particles, more than 2048 under NoCutoff, another particle count than the context's, the
 * parameter, variable and type limits, an index out of range, CutoffPeriodic without a box, a periodic cutoff above half the shortest
 * box edge (also at an evaluation, after the box has shrunk), more than one rank.  An ordinary member of a group, evaluated through
 * amm_force_eval and amm_run_ops, legal in a context without a box; every other family's entry points refuse its id naming
 * AMM_FORCE_MANY_PARTICLE.
 * Two launches per evaluation, one wavefront per particle each: the neighbour scan (all columns 64 at a time, the survivors
 * appended in ascending order to the particle's row of a table n x capacity -- with a cutoff the option "many_capacity",
 * amm_set_option, else n - 1 rounded up to 64) and the evaluation, in which the wavefront of particle i enumerates every set that
 * contains i, queues the survivors in LDS, runs the interpreter on full queues and adds the force on i alone: every set is
 * interpreted three times.  A row that needs more than the capacity is clamped and raises a flag that amm_check reports with both
 * numbers; the energy and forces of that evaluation are unspecified, but no access leaves the table.  No atomics: the same positions
 * give the same bits, with and without energy. */
int amm_many_create(amm_ctx *ctx, const int32_t *code, int32_t ncode, const double *consts, int32_t nconst, const double *globals,
                    int32_t nglobal, const int32_t *var_kinds, const int32_t *var_slots, int32_t n_vars, int32_t n_particles,
                    const double *h_params, int32_t n_params, const int32_t *h_types, int32_t n_types, const int32_t *h_perm,
                    const int32_t *h_excl, int32_t n_excl, double rc, int32_t periodic, int32_t central, int32_t *force_id);
/* setParticleParameters / setTypeFilter + updateParametersInContext: all per-particle values, the types and the permutation table
 * again, laid out as at creation (the same particle count; n_types may differ). */
int amm_many_set_params(amm_ctx *ctx, int32_t force_id, const double *h_params, int32_t n_particles, int32_t n_params,
                        const int32_t *h_types, int32_t n_types, const int32_t *h_perm);
/* Context.setParameter(name, value) for a global parameter of such a force: all of the program's globals, in its order. */
int amm_many_set_globals(amm_ctx *ctx, int32_t force_id, const double *globals, int32_t nglobal);
/* Waits for the stream.  out[0]: particles; out[1]: evaluations of the text whose energy the last evaluation summed (SinglePermutation:
 * the sets; UniqueCentralParticle: one per set and centre; 0 before the first); out[2]: kernel launches so far; out[3]: the fullest
 * neighbour row of the last evaluation, unclamped; out[4]: the capacity of a row. */
int amm_many_stats(amm_ctx *ctx, int32_t force_id, int64_t *out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_many_release(amm_ctx *ctx, int32_t force_id);

/* RMSDForce (force type AMM_FORCE_RMSD; csrc/rmsd.hip): the root-mean-square deviation, in nm, of the n_sel
 * particles h_particles from the reference rows h_ref[n_sel][3] (row k belongs to particle h_particles[k]) after the optimal rigid
 * superposition -- translation and PROPER rotation, by Horn's quaternion -- as an energy, with force -d_i / (n_sel rmsd) on
 * particle i, d_i its residual after the fit.  The library centres the reference in extended precision.  Positions are read raw: no
 * box, no minimum image.  A mean square deviation below 1e-20 nm^2 gives energy 0 and zero rows, never a NaN.
 * Refused, each with AMM_FORCE_RMSD in the message: n_sel < 1, an index outside [0, n), an index listed twice, a reference
 * coordinate that is not finite, more than one rank (also amm_set_slice while such a force lives).  An ordinary member of a group,
 * evaluated through amm_force_eval and amm_run_ops, legal in a context without a box, and a legal inner force of amm_cv_create; every
 * other family's entry points refuse its id naming AMM_FORCE_RMSD.
 * fp64, no atomics, fixed order of summation: the same positions give the same bits.  One launch of one block up to a selection size
 * measured on an MI355X, three launches of several blocks above it; the option "rmsd_blocks" (amm_set_option, read when the force is
 * created) forces either.  Without `accumulate` the rows of the particles outside the selection are written as zeros. */
int amm_rmsd_create(amm_ctx *ctx, const int32_t *h_particles, int32_t n_sel, const double *h_ref, int32_t *force_id);
/* setReferencePositions / setParticles + updateParametersInContext: new particles and / or a new reference, laid out as at creation;
 * n_sel may change.  Waits for the stream.  A refused call leaves the force as it was. */
int amm_rmsd_set_reference(amm_ctx *ctx, int32_t force_id, const int32_t *h_particles, int32_t n_sel, const double *h_ref);
/* out[0]: selected particles; out[1]: blocks (1: the single block); out[2]: launches per evaluation (1 or 3); out[3]: launches so far. */
int amm_rmsd_stats(amm_ctx *ctx, int32_t force_id, int64_t *out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_rmsd_release(amm_ctx *ctx, int32_t force_id);

/* GayBerneForce (force type AMM_FORCE_GAYBERNE; csrc/gayberne.hip): ellipsoids with the anisotropic pair
 * energy E = U eta chi S(r) of OpenMM's class, the frame of an ellipsoid defined by its x- and y-particle, the torque returned as
 * forces on those particles (the exact gradient, the roll of the frame about its x axis included).
 * The caller compacts the INTERACTING particles (epsilon > 0, or in an exception with epsilon > 0): marker atoms never enter the scan.
 *   h_active[n_active]      their particle indices, ascending
 *   h_axes[n_active][2]     x- and y-particle of the row (-1: none; no x-particle: a sphere; no y-particle: sy = sz and ey = ez)
 *   h_par[n_active][8]      sigma, epsilon, sx, sy, sz, ex, ey, ez (nm, kJ/mol, nm x 3, pure numbers)
 *   h_ex_ptr[n_active + 1], h_ex_col[], h_ex_par[][2]   the exceptions as a CSR over active rows: columns are active indices,
 *                           ascending within a row; (sigma, epsilon) per entry, epsilon 0 removes the pair; every pair on both rows
 *   h_rev_ptr[n + 1], h_rev_src[]   per particle of the context the entries 2 * row + (0: x-particle, 1: y-particle) that name it,
 *                           ascending: the order in which the spread adds them
 *   cutoff                  0: NoCutoff; above 0: pairs at r >= cutoff contribute nothing (no shift)
 *   switch_distance         below 0: none; else S = 1 - 10 t^3 + 15 t^4 - 6 t^5, t = (r - switch_distance) / (cutoff - switch_distance)
 *   periodic                minimum images for the pair AND for the frames; needs cutoff <= half the shortest box edge
 * Refused, each with AMM_FORCE_GAYBERNE in the message: more than 32768 active particles, an index out of range, an axis particle
 * that is the particle itself, a shape its axes cannot orient, tables that are not ordered or not consistent, a switching distance
 * outside [0, cutoff), more than one rank (also amm_set_slice while such a force lives).  An ordinary member of a group; no inner
 * force of amm_cv_create.  fp64, no atomics, fixed order of summation: the same positions give the same bits.  All pairs of active
 * particles are scanned, each pair evaluated from both sides; four launches per evaluation. */
int amm_gayberne_create(amm_ctx *ctx, const int32_t *h_active, int32_t n_active, const int32_t *h_axes, const double *h_par, const int32_t *h_ex_ptr,
                        const int32_t *h_ex_col, const double *h_ex_par, const int32_t *h_rev_ptr, const int32_t *h_rev_src, double cutoff,
                        double switch_distance, int32_t periodic, int32_t *force_id);
/* setParticleParameters / setExceptionParameters + updateParametersInContext: new values in the layout of creation; the counts, the
 * axes and the sparsity of the exceptions stay.  Waits for the stream.  A refused call leaves the force as it was. */
int amm_gayberne_set_params(amm_ctx *ctx, int32_t force_id, const double *h_par, int32_t n_active, const double *h_ex_par, int32_t n_entries);
/* out[0]: active rows; out[1]: ordered pairs an evaluation tests; out[2]: those that passed the cutoff and the exceptions in the last
 * evaluation (each pair from both sides); out[3]: launches so far; out[4]: chunks a row's columns are split into. */
int amm_gayberne_stats(amm_ctx *ctx, int32_t force_id, int64_t *out);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_gayberne_release(amm_ctx *ctx, int32_t force_id);

/* DrudeForce (force type AMM_FORCE_DRUDE; csrc/drude.hip): anisotropic harmonic springs between Drude
 * particles and their parents, and Thole-screened interactions between the dipoles of pairs of them, with K = 138.935456:
 *   spring  a1 = aniso12 if p2 != -1 else 1, a2 = aniso34 if p3, p4 != -1 else 1, a3 = 3 - a1 - a2, k3 = K q^2/(alpha a3),
 *           k1 = K q^2/(alpha a1) - k3, k2 = K q^2/(alpha a2) - k3, d = x_p - x_p1,
 *           E = 1/2 k3 |d|^2 + 1/2 k1 (d.unit(x_p1 - x_p2))^2 + 1/2 k2 (d.unit(x_p3 - x_p4))^2
 *   pair    s = thole/(alpha_A alpha_B)^(1/6); over the four site pairs of {p_A: q_A, p1_A: -q_A} x {p_B: q_B, p1_B: -q_B}, u = s r:
 *           E += K q_i q_j (1 - (1 + u/2) exp(-u))/r
 *   h_idx[n_drude][5]     p, p1, p2, p3, p4 (-1: none)
 *   h_par[n_drude][4]     charge (e), polarizability (nm^3), aniso12, aniso34
 *   h_pair[n_pairs][2]    the two entries of h_idx a screened pair joins;  h_thole[n_pairs]
 *   periodic              every displacement takes its own minimum image in the orthorhombic box
 * Refused, each with AMM_FORCE_DRUDE in the message: an index out of range, p = p1, a polarizability or an a1, a2, a3 that is not
 * above zero, a pair that names an entry twice or one that does not exist, more than one rank (also amm_set_slice while such a
 * force lives).  An ordinary member of a group; no inner force of amm_cv_create.  fp64, no atomics, fixed order of summation: the
 * same positions give the same bits.  Two launches per evaluation. */
int amm_drude_create(amm_ctx *ctx, const int32_t *h_idx, const double *h_par, int32_t n_drude, const int32_t *h_pair, const double *h_thole,
                     int32_t n_pairs, int32_t periodic, int32_t *force_id);
/* setParticleParameters / setScreenedPairParameters + updateParametersInContext: new values in the layout of creation; the counts and
 * every index stay.  Waits for the stream.  A refused call leaves the force as it was. */
int amm_drude_set_params(amm_ctx *ctx, int32_t force_id, const int32_t *h_idx, const double *h_par, int32_t n_drude, const int32_t *h_pair,
                         const double *h_thole, int32_t n_pairs);
/* Free such a force; the id is retired and leaves every group definition. */
int amm_drude_release(amm_ctx *ctx, int32_t force_id);

/* Reciprocal space of a NonbondedForce with nonbondedMethod PME / Ewald, as RESPASystem and FarNonbondedForce
 * keep it in group 2 with the source force's Ewald tolerance / PME parameters (systems.py:74-75,
 * forces.py:185-188; setReciprocalSpaceForceGroup: utils.py:147-152).  Smooth PME, B-spline order 5, grid
 * nx x ny x nz; the energy includes the Ewald self term (no neutralising-background term for a charged box: the
 * reference's literals have none, tests/test_systems.py:173).
 * Evaluated through amm_force_eval like the other force objects. */
int amm_pme_create(amm_ctx *ctx, double alpha, int32_t nx, int32_t ny, int32_t nz, double Kc, const double *h_q,
                   int32_t *force_id);
int amm_pme_set_charges(amm_ctx *ctx, int32_t force_id, const double *h_q);   /* parameter offsets on charges */
/* world > 1: gather forces only for this rank's block of atoms (use inside an all-reduced group). */
int amm_pme_set_sliced(amm_ctx *ctx, int32_t force_id, int32_t on);

/* Context.getState(getForces=True, getEnergy=True, groups=...)  (utils.py:159-164).
 * d_force [n][3]: overwritten (accumulate=0) or added to; d_energy: *d_energy += E (skipped if NULL). */
int amm_force_eval(amm_ctx *ctx, int32_t force_id, const double *d_pos, double *d_force,
                   int32_t accumulate, double *d_energy);

/* CustomIntegrator per-DOF steps as the reference emits them (propagators.py:249, 271; integrators.py:113). */
int amm_kick(amm_ctx *ctx, double *d_v, const double *d_f, const double *d_f2, int32_t plus, const double *d_mass, double coef);
int amm_move(amm_ctx *ctx, double *d_x, const double *d_v, double coef);
int amm_copy(amm_ctx *ctx, double *d_dst, const double *d_src);
int amm_mvv(amm_ctx *ctx, const double *d_v, const double *d_m, double *d_out); /* addComputeSum('mvv','m*v*v') */

/* CustomIntegrator.step(n)  (integrators.py:153-163): bind state buffers, define groups, run ops. */
/* CustomIntegrator.addComputePerDof(variable, expression) / addComputeSum(variable, expression) for expressions
 * beyond kick and move -- the thermostat / stochastic propagators (propagators.py:276-827, 1108-2172), and
 * integrators.py:113 `addComputeSum('mvv', 'm*v*v')`.  `code` is a postfix program (opcode | arg << 8; opcodes in
 * atomsmm_amd/expr.py and csrc/expr.hip) over constants, global variables, the bound per-DOF buffers (by slot), the
 * masses and `gaussian` / `uniform` draws (Philox-4x32-10 keyed by seed; counter = launch index).  d_dst ([n][3],
 * may be one of the bound buffers) receives the per-DOF values, *d_sum (device) their sum; either may be NULL. */
int amm_expr_eval(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts,
                  const double *globals, int32_t n_globals, uint64_t seed, uint64_t counter, double *d_dst, double *d_sum);

/* CustomIntegrator.addComputeGlobal(variable, expression) whose operands wait on device results -- the extended variable's scalar
 * block of AdiabaticDynamicsIntegrator (integrators.py:701-737: lambda moves, reflects, is thermostatted, all on sums of
 * deriv(energy, lambda) that kernels already enqueued will leave in device memory).  The postfix program is a sequence of
 * assignments, each closed by X_OUT dst: d_scalars[dst] <- the value on the stack; X_DEVG operands are other entries of d_scalars
 * (n_scalars doubles, device; later assignments see earlier ones); constants as in amm_expr_eval, no per-DOF operands, no random
 * draws (the host makes those); <= 640 words, <= 96 constants.  One thread on the context's stream; the host never waits. */
int amm_expr_eval_scalar(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts, double *d_scalars,
                         int32_t n_scalars);

/* System.addConstraint(i, j, distance) x n (forcefield.createSystem(constraints=HBonds, rigidWater=True) in the
 * reference's tests, tests/test_propagators.py:11-18).  Clusters of coupled constraints (<= 8 atoms, <= 16 constraints)
 * are solved by one thread each; tolerance as CustomIntegrator.getConstraintTolerance() (<= 0: 1e-5).  The new set replaces the
 * context's previous one; a refused call (a bad index or distance, a cluster beyond the limits) leaves the previous set in force.
 * The solvers are plain Gauss-Seidel sweeps (SHAKE / RATTLE) with a cap of 500 sweeps: trees converge in tens of sweeps, rigid
 * clusters with cycles slowly (a six-ring with its 1-3 distances needed up to 278 sweeps at a tolerance of 1e-13 and 110 at
 * 1e-5, a methyl group with its H-H distances 182 and 76, a rigid water 65 and 29: tests/test_constraint_cases_host.py). */
int amm_constraints_create(amm_ctx *ctx, const int32_t *h_pairs, const double *h_dist, int32_t n_constraints, double tolerance);
/* A new tolerance for the solvers of the existing constraint set (setConstraintTolerance of a bound integrator); <= 0: 1e-5. */
int amm_constraints_set_tolerance(amm_ctx *ctx, double tolerance);

/* Register a per-DOF expression with fixed globals for AMM_OP_EXPR; amm_expr_seed sets the random stream used by the
 * ops (integrator.setRandomNumberSeed, integrators.py:149-151) and restarts its counter. */
int amm_expr_define(amm_ctx *ctx, const int32_t *code, int32_t n_code, const double *consts, int32_t n_consts,
                    const double *globals, int32_t n_globals, int32_t *expr_id);
int amm_expr_seed(amm_ctx *ctx, uint64_t seed);
/* z = exp(-gamma * fraction * dt), kT in kJ/mol: the constants of one Ornstein-Uhlenbeck bath step for AMM_OP_BATH. */
int amm_bath_define(amm_ctx *ctx, double z, double kT, int32_t *bath_id);
/* One of OpenMM's stock integrators for AMM_OP_STOCK: kind 0 Verlet (leapfrog), 1 LangevinMiddle, 2 Langevin, 3 Brownian; dt in ps,
 * friction in 1/ps, kT in kJ/mol (csrc/stock.hip has the formulas).  Refused: an unknown kind, friction <= 0 for Brownian, a
 * negative friction or kT, a step size of 0 (three kinds divide by it).  The op itself is refused while the isokinetic or the regulated mode is on. */
enum { AMM_STOCK_VERLET = 0, AMM_STOCK_LANGEVIN_MIDDLE = 1, AMM_STOCK_LANGEVIN = 2, AMM_STOCK_BROWNIAN = 3 };
int amm_stock_define(amm_ctx *ctx, int32_t kind, double dt, double friction, double kT, int32_t *stock_id);
/* The step of a DrudeLangevinIntegrator for AMM_OP_DRUDE_STEP (csrc/drude.hip has the formulas):
 *   h_pairs[n_pairs][2]   (Drude particle, parent) of every pair; no particle in two pairs
 *   dt in ps; friction, kT of the ordinary atoms and of the pairs' centres of mass; drude_friction, drude_kT of the pairs' relative
 *   motion (1/ps, kJ/mol); max_distance: the hard wall in nm, 0: none.
 * A pair found beyond twice the hard wall after a step sets a flag: the next amm_check returns 2 with the message "Drude particle
 * moved too far beyond hard wall constraint" and clears it.  Refused: an index out of range or named twice, a negative friction,
 * kT or distance, a step size of 0, more than one rank.  The op itself is refused while the isokinetic or the regulated mode is on. */
int amm_drude_step_define(amm_ctx *ctx, const int32_t *h_pairs, int32_t n_pairs, double dt, double friction, double kT, double drude_friction,
                          double drude_kT, double max_distance, int32_t *step_id);
/* The Nose-Hoover-Langevin bath block of NHL_R_Integrator (integrators.py:272-330; MassiveNoseHooverLangevinPropagator,
 * propagators.py:1362-1449) as ONE AMM_OP_BATH: v <- v exp(-h w) ; w <- z w + sqrt(kT (1 - z^2)/Q) gaussian +
 * (m v^2 - kT)(1 - z)/(Q friction) ; v <- v exp(-h w), with the per-DOF thermostat velocities w in buffer slot `slot`
 * (h = fraction * dt of the two scalings, z = exp(-2 h friction)). */
int amm_bath_define_nhl(amm_ctx *ctx, double h, double z, double kT, double Q, double friction, int32_t slot, int32_t *bath_id);
/* SIN(R) with L = 1 (SIN_R_Integrator, integrators.py:358-416; MassiveIsokineticPropagator / SIN_R_Propagator,
 * propagators.py:276-355, 1045-1105).  amm_iso_define(on = 1) puts the context in isokinetic mode: every AMM_OP_KICK becomes
 *   v <- v cosh(z) + sqrt(LkT/m) sinh(z), z = coef F / sqrt(m LkT) ; H = sqrt(LkT/(m v^2 + Q1 v1^2/2)) ; v <- H v ; v1 <- H v1
 * with the per-DOF thermostat velocities v1 in buffer slot `slot_v1`.  amm_bath_define_sin registers the bath block between
 * the two half moves -- v1 <- v1 exp(-h v2) ; rescale ; v2 <- z v2 + sqrt(kT (1 - z^2)/Q2) gaussian + (Q1 v1^2 - kT)(1 - z)/
 * (Q2 friction) ; v1 <- v1 exp(-h v2) ; rescale -- as ONE AMM_OP_BATH (v2 in slot_v2; needs the isokinetic mode). */
int amm_iso_define(amm_ctx *ctx, int32_t on, double LkT, double Q1, int32_t slot_v1);
int amm_bath_define_sin(amm_ctx *ctx, double h, double z, double kT, double Q2, double friction, int32_t slot_v2, int32_t *bath_id);
/* Regulated dynamics (RegulatedTranslationPropagator and the regulated Nose-Hoover-Langevin baths, propagators.py:1537-2007).
 * amm_regulated_define(on = 1) puts the context in regulated mode: every AMM_OP_MOVE becomes
 *   x <- x + c tanh(alpha v / c) coef,  c = sqrt(an_kT / m)      (an_kT = alpha_n n kT)
 * so that no degree of freedom moves faster than c; the fused epilogues of the pair-force launches are not planned then.
 * amm_bath_define_regulated registers the bath block of one regulated propagator as ONE AMM_OP_BATH: kind 3 regulated massive,
 * 4 twice-regulated massive, 5 regulated atomic, 6 twice-regulated atomic Nose-Hoover-Langevin.  The block is
 *   [w <- w + G h ;] v <- S(v, w) ; w <- w z [+ G (1 - z)/friction] + omega sqrt(1 - z^2) gaussian ; v <- S(v, w) [; w <- w + G h]
 * (bracketed boosts with split = 1, the drift term without), h = (fraction/2) dt, z = exp(-friction fraction dt); G and the
 * scaling S as the reference writes them (an = alpha_n n; Q = kT tau^2, or 3 kT tau^2 for the atomic kinds).  w is the per-DOF
 * buffer slot_v_eta; the atomic kinds keep one w per atom in all three components and draw the gaussian of its x component. */
int amm_regulated_define(amm_ctx *ctx, int32_t on, double alpha, double an_kT);
int amm_bath_define_regulated(amm_ctx *ctx, int32_t kind, int32_t split, double h, double z, double kT, double Q, double omega,
                              double friction, double alpha, double an, int32_t slot_v_eta, int32_t *bath_id);

int amm_bind_state(amm_ctx *ctx, double *d_x, double *d_v, const double *d_mass);
#define AMM_MAX_SLOTS 64
#define AMM_SLOT_X 62   /* positions and velocities are addressable as buffers too (`x0 <- x`) */
#define AMM_SLOT_V 63
int amm_bind_buffer(amm_ctx *ctx, int32_t slot, double *d_buf);              /* per-DOF buffers f0.., _f2_, fm1 */
int amm_group_define(amm_ctx *ctx, int32_t group, int32_t slot, const int32_t *force_ids, int32_t n_forces);
int amm_run_ops(amm_ctx *ctx, const amm_op *ops, int32_t n_ops, int32_t repeat);
/* Dual Verlet list: an OUTER list (radius rc + skin_out, built from the cell list, rare) is PRUNED to the inner list
 * (rc + skin) that the traversal walks whenever an atom moved more than skin/2.  Applies to pair forces created later. */
int amm_set_outer_skin(amm_ctx *ctx, double skin_out);
/* Tuning and test options of a context (set before the first evaluation; never read from the environment).  Names:
 * "cluster" (1: molecule rows for three-site molecules on the force-only path, 0: per-atom rows everywhere), "hybrid" (1: molecule
 * rows also for waters that share the box with other atoms, the rest through per-atom rows), "small_group" (1: interaction-group
 * forces with a set of <= 128 atoms are evaluated without a neighbour list), "rest_skin_factor" (Verlet buffer of a hybrid list's
 * per-atom part as a multiple of its molecule rows' buffer, default 2; set before amm_pair_create), "mixed_terms", "tab" (tabulated
 * force-only kernels), "site_trips", "lanes_per_row", "build_parts", "build_split" (molecule rows: the split-stream
 * list build -- a block per (cell, part), both passes shared out over its four wavefronts; 0 = off (default: not faster than the
 * one-wavefront build on the slices measured), -1 = for a rank's slice of the rows, k = k blocks per cell; the rows are the same), "unroll", "dual_unroll", "tab_block", "tab_dual_block",
 * "terms_from", "no_term_lanes", "row_phases" (1: the rows a molecule-row traversal cannot deal out in whole
 * rounds of wavefront tasks go out in smaller tasks), "group_candidates" (1: a list-free group force on a fused inner loop walks only
 * the atoms near its small set while a neighbour list of the context vouches for them), "positions_private" (1: the caller promises
 * to call amm_positions_changed after writing the bound position buffer itself; amm_run_ops then trusts the displacement checks its
 * own launches made at the end of the previous call instead of assuming that anything may have moved), "fuse_epilogue" (1: a molecule-row
 * pair kernel runs the kicks and the inner RESPA loop that follow its EVAL in the step program as its epilogue when the innermost group
 * is one bond-list set of three-site molecules -- propagators.py:933-973 unrolled; 0: launches of their own), "comm_timeout" (seconds
 * amm_check / amm_synchronize / amm_comm_destroy wait for the stream while the context owns an RCCL communicator before they abort it and
 * fail; default 0 = no deadline, the asynchronous error alone is polled), "gb_lanes_per_row" (lanes that sum one row of the
 * generalized-Born passes: 0 = chosen from n as for free-space pair forces; 1, 2, 4 .. 64), "cgb_lanes_per_row" (the same for the
 * passes of a custom generalized-Born force), "hbond_chunks" (column chunks a row of a hydrogen-bond force created from now on is
 * split into, one wavefront each: 0 = chosen from the number of rows; 1 .. 512), "hbond_compact" (0: such a force runs the
 * interpreter after every batch of 64 columns that has a survivor instead of on full queues -- for measurements; default 1),
 * "many_capacity" (neighbours a row of a many-particle force with a cutoff created from now on can hold: a multiple of 64 from 64
 * to 4096; default 256), "rmsd_blocks" (blocks of an RMSD force created from now on: 0 = one block up to the measured crossover and
 * one per 1024 particles above it, 1 = the single block, 2 .. 1024 = that many; default 0).  Unknown names are an error. */
int amm_set_option(amm_ctx *ctx, const char *name, double value);
/* What amm_run_ops fused so far (statistics for tests and bench.py): out[0] = pair-kernel launches that carried the inner RESPA loop
 * of their molecules as an epilogue (the reference runs it as CustomIntegrator steps, propagators.py:933-973), out[1] = pair
 * evaluations that found their sorted copies written by the launch that moved the atoms (no gather launch), out[2] = of out[0], the
 * launches on a rank's slice that were followed by an exchange of positions and velocities instead of forces, out[3] = scheduling
 * decisions made so far: one per op or fused run of ops (an evaluation counts as one whatever it launches) -- not kernel launches. */
int amm_run_stats(amm_ctx *ctx, int64_t out[4]);
/* Who made those scheduling decisions (tests): out[0] = ops run on their own (the plain path), out[1..6] = decisions of the fusion rules
 * in the numbering of csrc/run_ops.hip -- 1 trailing kicks deferred, 2 component-parallel inner loop, 3 fused inner iteration, 4 one pass
 * for two evaluations, 5 term-parallel evaluation + kicks, 6 kicks + move; their sum is out[3] of amm_run_stats.  out[7] = evaluations
 * that were offered an epilogue plan; those whose launch carried it are out[0] of amm_run_stats. */
int amm_run_rule_stats(amm_ctx *ctx, int64_t out[8]);
/* amm_run_ops, resumable (several ranks whose collectives the HOST makes -- torch.distributed over gloo, or RCCL outside the library):
 * starts at op *cursor of the unrolled program (repetition * n_ops + index; 0 at first) and runs to the end (*cursor = repeat * n_ops)
 * or to the first exchanged evaluation that now waits for its exchange: the caller all-gathers the chunks of the exchange buffer,
 * calls amm_exchange_finish and calls again with the cursor it was given.  With a communicator of the library's own nothing is left
 * to the host and one call runs everything, as amm_run_ops does. */
int amm_run_ops_from(amm_ctx *ctx, const amm_op *ops, int32_t n_ops, int32_t repeat, int64_t *cursor);
/* The bound position buffer was written by the caller (needed only with option "positions_private"; harmless otherwise). */
int amm_positions_changed(amm_ctx *ctx);
/* slots of the cell-sorted order per rank (whole molecules of three: 3 ceil(ceil(n/3) / world)): the exchange buffer holds
 * world x 2 x per x 3 doubles and a chunk of a single / dual evaluation is [1 or 2][per][3] */
int amm_exchange_per(amm_ctx *ctx, int32_t *per);
/* amm_run_ops fuses KICK;MOVE;EVAL(bond-list group);KICK into one launch (bit-identical results); 0 disables. */
int amm_set_fuse_inner(amm_ctx *ctx, int32_t on);

/* ---- a box that changes: constant-pressure runs ------------------------------------------------- */
/* Context::setPeriodicBoxVectors of OpenMM on a live context (orthorhombic: the three edges), which MonteCarloBarostat calls at
 * every attempt and PressureComputer.import_configuration (computers.py:243) at every frame.  Legal between any two amm_run_ops /
 * amm_force_eval calls; stream-ordered -- every kernel takes the box by value at launch, so work already queued keeps the old one.
 * Every pair force derives its Verlet buffer and list radii again under the clamp skin <= 0.999 (L/2 - rc), every neighbour list,
 * sorted copy, candidate set and displacement reference made for the old box is dropped, and the next evaluation is exact for the
 * new one.  The cell counts of a list are kept, and nothing is sized, allocated or waited for, while (a) the cells still admit the
 * list radius -- a kept grid may take up to half of the Verlet buffer before it gives way, (b) the density of list entries
 * rlist^3 / V has grown by less than a quarter since the list was sized, and (c) the edges are within 2 % of those at that time or
 * the cell counts a fresh context would choose are the same.  Otherwise the list is dropped with its capacities and the next
 * evaluation sizes and builds it as a first evaluation does (a "regrid").  Non-zero with the message of amm_pair_create when a pair
 * force has rc > L/2 on some axis, or when a wait or an allocation fails: the old box then stays in force (lists that were already
 * dropped are built again by their next evaluation).  A list made with an outer buffer (amm_set_outer_skin) is sized again when the
 * clamp takes that buffer away or gives it back.  Not for a context that is one rank of several (nor is amm_mol_scale). */
int amm_set_box(amm_ctx *ctx, const double h_box[3]);
/* out[0] = amm_set_box calls that succeeded, out[1] = those that chose new cell counts for some list, out[2] = those that
 * freed or allocated device memory or waited for the stream, out[3] = 0. */
int amm_box_stats(amm_ctx *ctx, int64_t out[4]);
/* Context::getMolecules of OpenMM, handed over once: molecule m holds atoms h_atoms[h_ptr[m] .. h_ptr[m + 1]) (CSR, n_mol + 1
 * offsets).  Every atom of the context belongs to exactly one molecule -- anything else is an error; the atoms of a molecule need
 * not be contiguous.  Replaces an earlier definition (waits for the stream). */
int amm_mol_define(amm_ctx *ctx, const int32_t *h_ptr, const int32_t *h_atoms, int32_t n_mol);
/* The coordinate scaling of MonteCarloBarostat (ReferenceMonteCarloBarostat::applyBarostat of OpenMM): for every molecule, the centre
 * c = the unweighted mean of its atoms' positions, summed in list order with a fixed association (two runs give the same bits); every
 * atom of the molecule moves by (scale[k] - 1) c[k] along axis k.  d_x_saved (may be NULL) first receives the old positions bit for
 * bit: amm_copy from it undoes a rejected move.  Nothing is wrapped into the box.  One launch (csrc/barostat.hip: one lane per
 * molecule of up to 8 atoms, one wavefront per longer one); counts as amm_positions_changed. */
int amm_mol_scale(amm_ctx *ctx, double *d_x, double *d_x_saved, const double scale[3]);

/* ---- virtual sites and massless particles ------------------------------------------------------ */
/* System.setVirtualSite of OpenMM: a particle of mass 0 whose position is a function of up to three parents (the M site of TIP4P-class
 * water, the lone pairs of TIP5P or of a ligand).  csrc/vsite.hip; DESIGN.md section 3.VS.
 *   AMM_VSITE_AVERAGE2      TwoParticleAverageSite     s = w1 r1 + w2 r2                            weights (w1, w2, -)
 *   AMM_VSITE_AVERAGE3      ThreeParticleAverageSite   s = w1 r1 + w2 r2 + w3 r3                    weights (w1, w2, w3)
 *   AMM_VSITE_OUT_OF_PLANE  OutOfPlaneSite             s = r1 + w12 r12 + w13 r13 + wc (r12 x r13)  weights (w12, w13, wCross)
 * with r12 = r2 - r1, r13 = r3 - r1 taken as plain differences (no minimum image: the parents of a site belong to one molecule, and
 * molecules are never split across the box).  LocalCoordinatesSite is not offered.
 * amm_vsite_define: h_site[n_sites] the sites' atom indices, h_kind[n_sites], h_parents[3 n_sites] (a site of two parents pads with
 * -1), h_weights[3 n_sites].  Refused: an index out of range, an atom that is a site twice, a parent that is a site, a parent named
 * twice, an unknown kind, a weight that is not finite.  Replaces an earlier definition (waits for the stream); n_sites = 0 removes it.
 * amm_vsite_place: d_x [n][3], sites <- their parents; one launch over the sites, fp64 without contraction.  Other rows are not read
 *   or written.  No-op without sites.
 * amm_vsite_spread: the force each site collected in d_f goes to its parents (J^T f at the positions d_x) and the site's row becomes
 *   0: average sites f_k += w_k f; out-of-plane f2 += w12 f + wc (r13 x f), f3 += w13 f + wc (f x r12), f1 += f - those two.
 *   Owner-computes: one lane per parent atom adds its (site, role) entries in the order of the sites -- no atomics, the same bits
 *   from run to run; the rows of the sites are zeroed by a second launch.  No-op without sites.
 * While sites are defined, amm_run_ops (a) places them after every op that writes the bound positions (MOVE, STOCK, CONSTRAIN_X,
 * EXPR / COPY / COMBINE into them), as amm_move / amm_copy / amm_expr_eval do when they write the bound buffer; the displacement
 * check of the launch that moved the atoms has not seen the sites' new positions, so the neighbour lists run their own check;
 * (b) spreads a group's buffer after every EVAL; (c) runs every op on its own: no fusion rule and no epilogue plan applies.
 * amm_force_eval neither places nor spreads: its caller does.
 * Massless particles (sites or not) are skipped by what integrates: AMM_OP_KICK, AMM_OP_BATH's Ornstein-Uhlenbeck step and
 * AMM_OP_STOCK leave their rows as they are, and AMM_OP_EXPR / amm_expr_eval leave the destination of their degrees of freedom
 * unwritten and add nothing to its sum (OpenMM's computePerDof / computeSum rule).  The Nose-Hoover-Langevin, isokinetic and
 * regulated baths and kicks do not know them.  Nor do the FUSED launches of amm_run_ops (the inner loop, the pair kernels' epilogues,
 * kicks carried by a gather: they divide by every mass, and a massless row becomes NaN): the library keeps them out by itself only
 * while sites are defined -- a caller whose mass array holds a zero without any site calls amm_set_fuse_inner(ctx, 0), as the
 * engine does, and must not switch it back on.
 * amm_vsite_stats: out[0] = amm_vsite_place launches, out[1] = spreads (two launches each), out[2] = kernel launches of both,
 * out[3] = sites defined; counted since the last amm_vsite_define. */
enum { AMM_VSITE_AVERAGE2 = 0, AMM_VSITE_AVERAGE3 = 1, AMM_VSITE_OUT_OF_PLANE = 2 };
int amm_vsite_define(amm_ctx *ctx, int32_t n_sites, const int32_t *h_site, const int32_t *h_kind, const int32_t *h_parents,
                     const double *h_weights);
int amm_vsite_place(amm_ctx *ctx, double *d_x);
int amm_vsite_spread(amm_ctx *ctx, const double *d_x, double *d_f);
int amm_vsite_stats(amm_ctx *ctx, int64_t out[4]);

/* ---- energy minimisation --------------------------------------------------------------------- */
/* LocalEnergyMinimizer::minimize(context, tolerance, maxIterations) of OpenMM, which the reference reaches through
 * app.Simulation.minimizeEnergy (the line every AtomsMM script runs before simulation.step): OpenMM runs L-BFGS on the host over
 * positions it copies to and from the platform at every evaluation.  Here the L-BFGS vectors live on the device (csrc/minimize.hip,
 * Gram-matrix form of the two-loop recursion): the caller evaluates energies and forces with amm_force_eval, the object below keeps
 * the history of steps and gradient differences, makes search directions and trial positions, and hands the line search one block
 * of eight scalars per evaluation.  The line search itself (a few comparisons per evaluation) is the caller's.
 *
 * amm_min_create: memory = pairs (s, y) kept, 1 .. 8; max_step (nm; <= 0: 0.1) = the farthest any atom moves in one trial;
 * force_input = 1: the d_g arguments below hold FORCES (minus the gradient), as amm_force_eval leaves them; d_mass ([n], caller-owned,
 * may be NULL): atoms of mass 0 never move and their gradient counts as zero (OpenMM's massless particles); d_scalars: 8 doubles of
 * device memory, caller-owned, zeroed here --
 *   [0] E         the caller's evaluations ADD the energy here (amm_force_eval's d_energy); amm_min_trial sets it to 0
 *   [1] g.d       slope along the current direction (< 0)          [2] g.g over the free components
 *   [3] max|g_i|  over the free components                         [4] 1 if the newest pair failed the curvature test
 *   [5] pairs in use (0: d = -g)                                   [6] the step factor the last amm_min_trial used
 *   [7] largest |d_atom|^2 over the atoms
 * Sums are fixed-order: two runs give the same bits.  Everything is enqueued on the context's stream; only amm_min_scalars,
 * amm_min_stats, amm_min_read and amm_min_release wait for it. */
int amm_min_create(amm_ctx *ctx, int32_t memory, double max_step, int32_t force_input, const double *d_mass, double *d_scalars,
                   int32_t *min_id);
int amm_min_release(amm_ctx *ctx, int32_t min_id);
/* Start at (d_x, d_g): x_prev <- x, g_prev <- g, history cleared, direction d = -g.  With d_x = d_g = NULL: keep the stored point,
 * clear the history and return to d = -g (the restart of a line search that found no step).  lbfgs() start / restart. */
int amm_min_begin(amm_ctx *ctx, int32_t min_id, const double *d_x, const double *d_g);
/* The accepted point (d_x, d_g): the pair s = x - x_prev, y = g - g_prev enters the ring (it is dropped again if s.y <= 1e-10 |s||y|),
 * x_prev <- x, g_prev <- g, and the object's direction buffer receives d = -H g of the two-loop recursion with H0 = (s.y / y.y) I of
 * the newest pair; d = -g if that is no descent direction.  Three launches: Gram update, coefficients, combination. */
int amm_min_advance(amm_ctx *ctx, int32_t min_id, const double *d_x, const double *d_g);
/* d_x_out <- x_prev + a d with a = min(alpha, max_step / largest |d_atom|); atoms of mass 0 (and alpha = 0) copy x_prev bit for bit.
 * One launch. */
int amm_min_trial(amm_ctx *ctx, int32_t min_id, double alpha, double *d_x_out);
/* The scalar block, after waiting for the stream: the one synchronisation of an energy evaluation. */
int amm_min_scalars(amm_ctx *ctx, int32_t min_id, double out[8]);
/* out[0] = pairs formed (amm_min_advance calls), [1] = trials, [2] = pairs dropped by the curvature test, [3] = restarts
 * (amm_min_begin without arguments), [4] = directions replaced by -g because g.d >= 0, [5] = pairs in use, [6] = memory.  Synchronises. */
int amm_min_stats(amm_ctx *ctx, int32_t min_id, int64_t out[8]);
/* Test and inspection access (host memory out; synchronises): what = 0 the matrix of dot products, (2m+1)^2 doubles over
 * [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g] by ring slot; 1 the coefficients delta, 2m+1; 2 the direction d, 3n. */
int amm_min_read(amm_ctx *ctx, int32_t min_id, int32_t what, double *h_out);

/* ---- measurement ----------------------------------------------------------------------------- */
typedef struct {
    int64_t n_builds;       /* neighbour-list (re)builds so far                       */
    int64_t n_evals;        /* force evaluations so far                               */
    int64_t n_list_pairs;   /* directed pairs currently in the list (this slice)      */
    int64_t n_slice_atoms;  /* atoms owned by this rank's slice                       */
    int32_t capacity;       /* neighbour slots per atom                               */
    int32_t max_neighbors;  /* longest list                                           */
    int32_t lanes_per_atom; /* lanes of a wavefront that share one i-atom             */
    int32_t n_cells;
    double rlist;
    int32_t shares_list;    /* 1 if this force traverses another force's list */
    int32_t list_kind;      /* rows walked by the last evaluation: 0 one per atom, 1 one per molecule (three-site molecules only,
                               force-only evaluations: n_list_pairs then counts nine atom pairs per entry, capacity and
                               max_neighbors are molecule partners per row, lanes_per_atom is lanes per row), 2 hybrid: one per
                               three-site molecule for the pairs of two molecules + one per atom, filtered to the pairs with an
                               atom outside the molecules, for the rest (an ion, a solute, a chain next to the waters), 3 none:
                               an interaction-group force whose smaller set has <= 128 atoms is evaluated without a list,
                               4 none: a free-space force (AMM_FREE_SPACE) walks all pairs; lanes_per_atom is its lanes per row */
    int64_t n_outer_builds; /* cell-based builds of the outer list (n_builds counts prunes of the inner list) */
    int64_t n_outer_pairs;
    double rlist_outer;
    double tab_error;       /* largest relative interpolation error of the force's radial Coulomb table at its check points;
                               0 without a table (analytic kernels: family without one, or a table that missed 1e-13) */
    int32_t has_table;
    int32_t rode_along;     /* 1: this force's last force-only evaluation was computed inside its list owner's launch (molecule rows:
                               the fused step-boundary pass), so it has no launch and no profile time of its own */
    int32_t has_site_table; /* 1: pairs of two Lennard-Jones sites read a radial table of their own in the molecule-row kernels (the
                               force's sites share one sigma, eps and charge: water) instead of Lennard-Jones arithmetic */
    int32_t n_rest_atoms;   /* hybrid lists: atoms outside the three-site molecules (0: none, or the force keeps per-atom rows) */
    double site_tab_error;  /* its largest relative interpolation error (bound 3e-13: the r^-14 wall) */
    int32_t n_candidates;   /* list_kind 3 on a fused inner loop: atoms within cutoff + buffer of the small set at the companion
                               list's last build (the later evaluations walk these only); 0: every evaluation walks every atom */
    int32_t n_candidate_walks;  /* evaluations that walked the candidates only */
    int32_t chargeless;         /* 1: the last force-only evaluation ran the per-atom-row kernel's instantiation without the Coulomb
                                   table (every charge of the force is zero: the Lennard-Jones fluid of BASELINE config C2) */
    int32_t build_split;        /* molecule rows: blocks per cell of the split-stream list build (a rank's slice of the rows: the four
                                   wavefronts of a block share one cell's candidate stream); 0: one wavefront per (cell, part) */
} amm_pair_stats;
int amm_pair_get_stats(amm_ctx *ctx, int32_t force_id, amm_pair_stats *out);   /* synchronises */
/* Measurement helper (bench.py): the number of directed list entries of this force with r < r_within at d_pos, counted in
 * fp64 by one launch over the neighbour rows (an evaluation must have built them).  Half of it is the number of pairs the
 * reference's expression is evaluated for when r_within is the force's cutoff (forces.py:659-661).  Synchronises. */
int amm_pair_count_within(amm_ctx *ctx, int32_t force_id, const double *d_pos, double r_within, int64_t *count);
/* Measurement helper (bench.py): molecule rows -- out[0] = lane-trips the traversal of this force executes (a wavefront walks
   64 / lanes_per_row rows until the longest is done), out[1] = row entries; their ratio is the padding of the walk.  Zeros for
   per-atom rows.  Synchronises. */
int amm_pair_row_padding(amm_ctx *ctx, int32_t force_id, int64_t out[2]);
/* A force whose last force-only evaluation rode on its list owner's fused pass (amm_pair_stats::rode_along): out[0] = its factor
   relative to the host, (Kc sign)_guest / (Kc sign)_host, out[1] = 1.0 if the launch took the kernel that leaves the product by a
   factor of exactly 1.0 out, else 0.0.  Zeros for a force that never rode along. */
int amm_pair_guest_factor(amm_ctx *ctx, int32_t force_id, double out[2]);
/* Revision tag of the pair-traversal kernels: measurements kept under profiles/ carry it, and bench.py drops a stored
 * figure (the PMC traffic) once the kernels it was measured on have changed. */
const char *amm_kernel_revision(void);
/* Host-only check of a descriptor's radial tables (no device is touched): builds the Coulomb table -- and, for sites of one
 * (sigma, eps, q), site_eps > 0, the site-site table -- as amm_pair_create does, and forms the interval index WITHOUT the clamp, as
 * the molecule-row kernels do for a pair that counts, at r2 = r2min, the next double, every interval boundary +- 2 ulp and the
 * last double below rc^2 (site pairs: from ss_r2min).  out = { intervals, first interval of the site-site table or -1, points
 * tested, points whose index fell outside the table, smallest index, largest index, intervals below the kink, refinement level of
 * the switching zone }.  out[3] must be 0: amm_pair_create drops a table for which it is not (analytic kernels). */
int amm_pair_table_check(const amm_pair_desc *desc, double site_sigma, double site_eps, double site_q, int64_t out[8]);
/* HIP-event timing of the dominant kernel (pair traversal) on the context stream. */
/* on = 1: HIP events around every pair-kernel launch; on = -(force_id + 1): only around that force's launches
 * (two event packets per timed launch cost ~4 us of stream time each: time what you report); 0: off. */
int amm_profile_enable(amm_ctx *ctx, int32_t on);
int amm_profile_read(amm_ctx *ctx, int32_t force_id, int64_t *n_launches, double *total_ms); /* synchronises, resets */

#ifdef __cplusplus
}
#endif
#endif
