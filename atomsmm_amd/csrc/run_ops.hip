// atomsmm_amd/csrc/run_ops.hip -- the op scheduler behind amm_run_ops / amm_run_ops_from: which ops of an integrator program share a
// launch.  One struct holds a run's state (OpRun), one member function per fusion rule; OpRun::step lists the rules in their order.
#include <algorithm>

#include "amm_ctx.h"
#include "expr_vm.h"

namespace {

// what a rule (and every helper that can end the run) answers; DONE / FAILED are the library's 0 / 1, so AMM_HIP works inside a rule
enum : int { DONE = 0, FAILED = 1, NOT_MINE = 2, YIELDED = 3 };

struct OpRun {
    amm_ctx *const ctx;
    const amm_op *const ops;
    const int n_ops, repeat;
    int64_t *const cursor;
    const long total_ops;
    int rep = 0;                    // the repetition that is running
    int k_start = 0;                // where the NEXT repetition starts (a wrapped plan covered its first ops)
    bool yielded = false;
    // kicks that close one repetition of the program ride on the first inner-loop launch of the next (as further
    // "preceding kicks"): same order, same arithmetic, two launches less per outer step.  Indices into ops; never more than three.
    int deferred[4], ndef = 0;
    // user-visible buffers; the fused inner iteration ping-pongs between them and library-owned partners
    double *const user_x, *const user_v;
    double *user_f0 = nullptr;
    int f0_slot = -1;
    bool swapped = false;
    bool restored = false;

    OpRun(amm_ctx *c, const amm_op *o, int n, int r, int64_t *cur)
        : ctx(c), ops(o), n_ops(n), repeat(r), cursor(cur), total_ops((long)r * n), user_x(c->d_x), user_v(c->d_v) {}
    // Every exit -- also the early `return 1` of a failed launch, an unbound buffer or a failed collective -- must leave the
    // context bound to the CALLER's buffers: the fused inner iteration ping-pongs d_x / d_v / the group-0 slot onto the
    // library's alt_* buffers.  On the error path the state held in the alt buffers is copied back on a best-effort basis.
    ~OpRun() { restore(true); }
    void restore(bool copy_back) {
        if (restored) return;
        restored = true;
        if (f0_slot < 0) return;
        if (swapped && copy_back) {
            const size_t bytes = sizeof(double) * 3 * (size_t)ctx->n;
            (void)hipMemcpyAsync(user_x, ctx->d_x, bytes, hipMemcpyDeviceToDevice, ctx->stream);
            (void)hipMemcpyAsync(user_v, ctx->d_v, bytes, hipMemcpyDeviceToDevice, ctx->stream);
            (void)hipMemcpyAsync(user_f0, ctx->slots[f0_slot], bytes, hipMemcpyDeviceToDevice, ctx->stream);
        }
        ctx->d_x = user_x;
        ctx->d_v = user_v;
        ctx->slots[f0_slot] = user_f0;
        ctx->slots[AMM_SLOT_X] = user_x;
        ctx->slots[AMM_SLOT_V] = user_v;
    }

    // ---- helpers, each written once ----
    double *slot(int i) const { return (i >= 0 && i < AMM_MAX_SLOTS) ? ctx->slots[i] : nullptr; }
    GroupDef *group(int g) const { return (g >= 0 && g < AMM_MAX_GROUPS) ? &ctx->groups[g] : nullptr; }
    long pos(int r, int k) const { return (long)r * n_ops + k; }
    bool is_kick(int k) const { return k < n_ops && ops[k].op == AMM_OP_KICK; }
    // the group's first member when that is a pair force (further members are added after its pass)
    PairForce *first_pair(const GroupDef &g) const {
        return !g.forces.empty() ? ctx->forces[g.forces[0]].pair() : nullptr;
    }
    // the group is exactly one pair force with a neighbour list (a free-space force has none: no plan rides on it, no slices)
    PairForce *sole_listed_pair(const GroupDef &g) const {
        PairForce *pf = g.forces.size() == 1 ? first_pair(g) : nullptr;
        return pf && !pf->free_space ? pf : nullptr;
    }
    // the group is exactly one bond-list set that this rank evaluates for every atom (a sliced set on several ranks: its rows only)
    BondedSet *sole_unsliced_bonded(const GroupDef &g) const {
        BondedSet *bs = g.forces.size() == 1 ? ctx->forces[g.forces[0]].bonded() : nullptr;
        return bs && bs->sliced && ctx->world > 1 ? nullptr : bs;
    }
    // The buffers of a run of kicks: the deferred kicks first (`lead`), then ops[from, to) -- all KICKs -- appended at index n of
    // fa / fb / plus / coef.  Stops at the first kick with an unbound buffer and answers false; what follows is the caller's to decide
    // (a rule declines and leaves the plain path to report it, flush_deferred reports it itself).
    bool bind_kicks(bool lead, int from, int to, const double **fa, const double **fb, int *plus, double *coef, int &n) const {
        const int nlead = lead ? ndef : 0, total = nlead + std::max(to - from, 0);
        for (int i = 0; i < total; ++i) {
            const amm_op &ko = ops[i < nlead ? deferred[i] : from + i - nlead];
            const double *a = slot(ko.a), *b = slot(ko.b);
            if (!a || (ko.b >= 0 && !b)) return false;
            fa[n] = a;
            fb[n] = b;
            plus[n] = ko.c;
            coef[n] = ko.coef;
            ++n;
        }
        return true;
    }
    // Behind an op that wrote the bound positions: virtual sites follow their parents at once (OpenMM places after every position
    // update; an evaluation never places), then the epoch moves on -- once, for the positions as they now stand.
    int x_written() {
        if (amm_vsite_place_impl(ctx, ctx->d_x)) return FAILED;          // (nothing without sites)
        ctx->pos_epoch++;
        return DONE;
    }
    bool in_own_only(const double *b) const { return b && std::find(ctx->own_only.begin(), ctx->own_only.end(), b) != ctx->own_only.end(); }
    // Buffers that hold this rank's rows only (state exchange, cluster.hip).  complete(buf): before an op reads `buf` for ALL atoms --
    // a bond-list group's buffer is evaluated again (every rank can: positions are whole after every exchange; the same numbers the
    // owners hold), anything else is an error: a pair group must be evaluated again before its forces are read.
    void forget_own_only(const double *buf) {
        auto it = std::find(ctx->own_only.begin(), ctx->own_only.end(), buf);
        if (it != ctx->own_only.end()) ctx->own_only.erase(it);
    }
    int complete(const double *buf) {
        if (ctx->own_only.empty() || !in_own_only(buf)) return DONE;
        for (int gi = 0; gi < AMM_MAX_GROUPS; ++gi) {
            GroupDef &g = ctx->groups[gi];
            if (g.slot < 0 || ctx->slots[g.slot] != buf || g.forces.empty()) continue;
            bool bonded_only = true;
            for (int fid : g.forces) bonded_only = bonded_only && ctx->forces[fid].bonded() && !ctx->forces[fid].bonded()->sliced;
            if (!bonded_only) break;
            bool first = true;
            for (int fid : g.forces) {
                if (amm_bonded_eval_impl(ctx, ctx->forces[fid].bonded(), ctx->d_x, ctx->slots[g.slot], first ? 0 : 1, nullptr)) return FAILED;
                first = false;
            }
            forget_own_only(buf);
            return DONE;
        }
        amm_set_error("amm_run_ops: an op reads a force buffer that holds this rank's rows only (state exchange) before its group was evaluated again");
        return FAILED;
    }
    int complete_all(const double *const *fa, const double *const *fb, int n) {
        for (int q = 0; q < n; ++q)
            if (complete(fa[q]) || complete(fb[q])) return FAILED;
        return DONE;
    }
    int flush_deferred() {
        const double *fa[4], *fb[4];
        int plus[4], n = 0;
        double coef[4];
        const bool bound = bind_kicks(true, 0, 0, fa, fb, plus, coef, n);
        for (int q = 0; q < n; ++q) {
            if (!ctx->own_only.empty() && (in_own_only(fa[q]) || in_own_only(fb[q]))) {
                amm_set_error("amm_run_ops: a deferred kick reads a force buffer that holds this rank's rows only (state exchange)");
                return FAILED;
            }
            if (amm_kick_impl(ctx, ctx->d_v, fa[q], fb[q], plus[q], ctx->d_mass, coef[q])) return FAILED;
        }
        if (!bound) {
            amm_set_error("amm_run_ops: KICK buffer not bound");
            return FAILED;
        }
        ndef = 0;
        return DONE;
    }
    int copy_op(const amm_op &op, bool whole_source) {
        double *dst = slot(op.a), *src = slot(op.b);
        if (!dst || !src) {
            amm_set_error("amm_run_ops: COPY buffer not bound");
            return FAILED;
        }
        if (whole_source && complete(src)) return FAILED;
        return amm_copy_impl(ctx, dst, src) ? FAILED : DONE;
    }
    // leave to the host what only it can do: an exchange pending without a communicator of the library's own.  DONE: go on,
    // YIELDED: *cursor is set -- wind up and return
    int leave_to_host(long next_pos) {
        if (!ctx->pending.active) return DONE;
        if (cursor) {
            *cursor = next_pos;
            return YIELDED;
        }
        if (next_pos == total_ops) return DONE;       // (the plain entry point: the caller finishes the exchange of the program's last op)
        amm_set_error("amm_run_ops: without a communicator (amm_comm_init) an exchanged EVAL must be the last op of the call (or use amm_run_ops_from)");
        return FAILED;
    }
    // After an evaluation that was offered a plan (ctx->epi_request).  Its launch carried the plan: go on behind the ops the plan
    // covered -- op q_resume, of the next repetition when the plan wrapped -- and answer DONE.  It did not: its buffers w1 / w2 are
    // written in full (by the kernel, or by the exchange's unsort), and NOT_MINE tells the caller to go on behind the evaluation
    // itself (op k_behind) with what else it has to do.  Either way the host may have an exchange to make first.
    int after_planned_eval(int &k, int q_resume, bool wraps, int k_behind, const double *w1, const double *w2) {
        if (ctx->epi_done) {
            ctx->epi_done = false;
            if (const int lv = leave_to_host(pos(wraps ? rep + 1 : rep, q_resume))) return lv;
            if (wraps) k_start = q_resume;
            k = wraps ? n_ops : q_resume;          // (wrapped: leaves the loop over this repetition's ops)
            return DONE;
        }
        forget_own_only(w1);
        if (w2) forget_own_only(w2);
        if (const int lv = leave_to_host(pos(rep, k_behind))) return lv;
        return NOT_MINE;
    }

    // ---- epilogue plans ----
    // (regulated mode: the epilogue's moves are plain ones -- not planned, the ops run on the paths that know the mode)
    bool plans_allowed() const { return !ctx->vsites && ctx->fuse_inner && ctx->opt_fuse_epilogue && !ctx->iso.on && !ctx->reg.on && !swapped && f0_slot < 0; }
    // The run of at most `cap` kicks at op `after`.  When the program ENDS with them (the closing half kicks of an outer step) and
    // another repetition follows, the run goes on with the kicks that open that repetition (`wraps`; what the deferred kicks do for
    // the stand-alone launches).  Answers their number; j: the op behind the run.
    int kick_run(int after, int cap, int &j, bool &wraps) const {
        int nk = 0;
        j = after;
        wraps = false;
        while (true) {
            while (is_kick(j) && nk < cap) { ++nk; ++j; }
            if (j == n_ops && !wraps && rep + 1 < repeat && nk > 0 && ops[0].op == AMM_OP_KICK) {
                wraps = true;
                j = 0;
                continue;
            }
            break;
        }
        return nk;
    }
    // ... and its first npre kicks as the plan's preceding kicks; false: one of their buffers is not bound (no plan)
    bool bind_plan_kicks(EpiPlan &P, int after, bool wraps, int npre) const {
        const int n1 = wraps ? std::min(npre, n_ops - after) : npre;
        P.npre = 0;
        return bind_kicks(false, after, after + n1, P.pre_a, P.pre_b, P.pre_plus, P.pre_coef, P.npre) &&
               bind_kicks(false, 0, npre - n1, P.pre_a, P.pre_b, P.pre_plus, P.pre_coef, P.npre);
    }
    // The force whose sorted copies the next pair evaluation reads (EpiPlan::next; nullptr: not known): that of the next EVAL in program
    // order from op `from`, across the end of the repetition (`wraps`: the plan reaches into the next one already).
    //   sole_member: the group must be that force alone.  Per-atom rows ask for it: their epilogue writes copies for the next evaluation
    //     of the launch's OWN force only, and that force is evaluated on this path only as a group's single member.  Molecule rows do not:
    //     a group's first member is evaluated first and reads the copies; the others (bond lists, reciprocal space) are added afterwards.
    //   prefer_list_owner: of two adjacent EVALs that run as one pass (rule_dual_eval), take the owner of the list: the pass walks the
    //     owner's list and reads the owner's copies.  Per-atom-row plans never sit in front of such a pair's shared pass.
    PairForce *next_pair_eval(int from, bool wraps, bool sole_member, bool prefer_list_owner) const {
        for (int t = from, seen = 0; seen < n_ops; ++seen, ++t) {
            if (t >= n_ops) {
                if (rep + (wraps ? 2 : 1) >= repeat) break;
                t = 0;
            }
            if (ops[t].op != AMM_OP_EVAL) continue;
            const GroupDef *ga = group(ops[t].a);
            PairForce *pa = !ga ? nullptr : sole_member ? sole_listed_pair(*ga) : first_pair(*ga);
            if (!pa || pa->free_space) break;          // (a free-space force reads no sorted copies)
            const GroupDef *gb = prefer_list_owner && t + 1 < n_ops && ops[t + 1].op == AMM_OP_EVAL ? group(ops[t + 1].a) : nullptr;
            PairForce *pb = gb ? first_pair(*gb) : nullptr;
            return pb && pa->host == pb ? pb : pa;
        }
        return nullptr;
    }
    // Molecule rows (cluster.hip: cepi_rows).  The ops that follow a force-only pair evaluation at op index `after` --
    // [KICK ...] ; n x { KICK(f0) ; MOVE ; EVAL(g0) ; KICK(f0) } with g0 = one bond-list set of three-site molecules -- as a plan the
    // evaluation's launch can carry.  q_resume: the first op not covered (in the next repetition when wraps).
    bool plan_epilogue(int after, EpiPlan &P, int &q_resume, bool &wraps) const {
        if (!plans_allowed()) return false;
        int j;
        const int nk = kick_run(after, AMM_MAX_PRE + 1, j, wraps);
        // the last kick of the run opens the first inner iteration
        if (nk == 0 || j < 1 || j + 2 >= n_ops) return false;
        const int start = j - 1;
        const amm_op &k1 = ops[start];
        if (!(k1.op == AMM_OP_KICK && k1.b < 0 && ops[start + 1].op == AMM_OP_MOVE && ops[start + 2].op == AMM_OP_EVAL &&
              ops[start + 3].op == AMM_OP_KICK)) return false;
        const int g0 = ops[start + 2].a;
        const GroupDef *g = group(g0);
        BondedSet *bs = g && g->slot == k1.a && !g->exchange ? sole_unsliced_bonded(*g) : nullptr;
        if (!bs || !bs->mol3_ok || bs->sliced) return false;
        auto is_iter = [&](int q) {
            return q + 3 < n_ops && ops[q].op == AMM_OP_KICK && ops[q].b < 0 && ops[q].a == k1.a && ops[q].coef == k1.coef &&
                   ops[q + 1].op == AMM_OP_MOVE && ops[q + 1].coef == ops[start + 1].coef && ops[q + 2].op == AMM_OP_EVAL &&
                   ops[q + 2].a == g0 && ops[q + 3].op == AMM_OP_KICK && ops[q + 3].b < 0 && ops[q + 3].a == k1.a &&
                   ops[q + 3].coef == ops[start + 3].coef;
        };
        int niter = 0, q = start;
        while (is_iter(q)) { ++niter; q += 4; }
        if (niter < 1 || nk - 1 > AMM_MAX_PRE) return false;
        P = EpiPlan();
        if (!bind_plan_kicks(P, after, wraps, nk - 1)) return false;
        P.bs = bs;
        P.f0 = slot(g->slot);
        P.niter = niter;
        P.c1 = k1.coef;
        P.d = ops[start + 1].coef;
        P.c2 = ops[start + 3].coef;
        if (!P.f0) return false;
        P.next = next_pair_eval(q, wraps, false, true);
        q_resume = q;
        return true;
    }
    // ... and for per-atom rows (pair.hip: AtomEpiArgs): `[KICK ...] [; MOVE]` behind the EVAL of a group that is one pair force -- a
    // velocity-Verlet step's closing half kick and, across the end of the repetition, the opening half kick + move of the next
    bool plan_atoms(int after, EpiPlan &P, int &q_resume, bool &wraps) const {
        if (!plans_allowed() || ctx->world != 1) return false;
        int j;
        const int nk = kick_run(after, 4, j, wraps);
        if (nk == 0 || is_kick(j)) return false;                                           // (a fifth kick: left to the plain path)
        const bool moves = j < n_ops && ops[j].op == AMM_OP_MOVE;
        if (!moves && !wraps && j == n_ops) return false;                                  // (closing kicks of the call's last step: as before)
        P = EpiPlan();
        P.kind = 1;
        if (!bind_plan_kicks(P, after, wraps, nk)) return false;
        P.with_move = moves ? 1 : 0;
        P.dcoef = moves ? ops[j].coef : 0.0;
        q_resume = moves ? j + 1 : j;
        P.next = next_pair_eval(q_resume, wraps, true, false);
        return q_resume < n_ops || !wraps;        // (a wrapped plan that swallowed the whole next repetition: not a step program)
    }

    // ---- the fusion rules: each looks at op k and answers NOT_MINE, DONE (k advanced), FAILED or YIELDED ----
    // 1. trailing block of the program = only KICKs and COPYs, and the program opens with KICKs: defer the kicks
    int rule_defer_trailing_kicks(int &k) {
        if (!(ctx->fuse_inner && !swapped && f0_slot < 0 && rep + 1 < repeat && k > 0 && ops[k].op == AMM_OP_KICK && ndef == 0 &&
              ops[0].op == AMM_OP_KICK)) return NOT_MINE;
        bool safe = true;
        int nk = 0;
        for (int j = k; j < n_ops && safe; ++j) {
            if (ops[j].op == AMM_OP_KICK) ++nk;
            else if (ops[j].op == AMM_OP_COPY) {
                // the copy runs now, the kicks before it later: it must not feed or clobber what they read
                if (ops[j].a >= AMM_SLOT_X || ops[j].b >= AMM_SLOT_X) safe = false;
                for (int i = k; i < j; ++i)
                    if (ops[i].op == AMM_OP_KICK && (ops[i].a == ops[j].a || ops[i].b == ops[j].a)) safe = false;
            } else safe = false;
        }
        if (!safe || nk > 3) return NOT_MINE;
        for (int j = k; j < n_ops; ++j) {
            if (ops[j].op == AMM_OP_KICK) deferred[ndef++] = j;
            else if (copy_op(ops[j], false)) return FAILED;
        }
        k = n_ops;          // next repetition
        return DONE;
    }
    // 2. component-parallel inner loop: [preceding KICKs] + n x {KICK(c1, fg) ; MOVE(d) ; EVAL(g) ; KICK(c2, fg)} in one launch
    int rule_inner_components(int &k) {
        if (!(ctx->fuse_inner && !swapped && ops[k].op == AMM_OP_KICK)) return NOT_MINE;
        int p = k, npre = 0;
        while (is_kick(p) && npre < 4) { ++p; ++npre; }
        // the last KICK of the run is the first op of the inner pattern
        const int start = p - 1;
        npre -= 1;
        // iteration = KICK(c1, fg) ; MOVE(d) ; [BATH(b) ; MOVE(d2) ;] EVAL(g) ; KICK(c2, fg)
        const bool bathed = start + 5 < n_ops && ops[start + 2].op == AMM_OP_BATH && ops[start + 3].op == AMM_OP_MOVE;
        const int stride = bathed ? 6 : 4, eo = bathed ? 4 : 2;       // ops per iteration / offset of the EVAL
        auto is_iter = [&](int q) {
            if (!(q + stride - 1 < n_ops && ops[q].op == AMM_OP_KICK && ops[q].b < 0 && ops[q + 1].op == AMM_OP_MOVE &&
                  ops[q + eo].op == AMM_OP_EVAL && ops[q + eo + 1].op == AMM_OP_KICK && ops[q + eo + 1].b < 0 &&
                  ops[q + eo + 1].a == ops[q].a && ops[q].a == ops[start].a && ops[q].coef == ops[start].coef &&
                  ops[q + 1].coef == ops[start + 1].coef && ops[q + eo + 1].coef == ops[start + eo + 1].coef &&
                  ops[q + eo].a == ops[start + eo].a))
                return false;
            if (bathed)
                return ops[q + 2].op == AMM_OP_BATH && ops[q + 2].a == ops[start + 2].a && ops[q + 2].a >= 0 &&
                       ops[q + 2].a < (int)ctx->baths.size() && ops[q + 3].op == AMM_OP_MOVE && ops[q + 3].coef == ops[start + 3].coef;
            return true;
        };
        const GroupDef *g = npre <= 3 && start >= k && is_iter(start) ? group(ops[start + eo].a) : nullptr;
        BondedSet *bs = g && g->slot == ops[start].a ? sole_unsliced_bonded(*g) : nullptr;
        if (bs && bs->max_comp <= 8) {
            int niter = 0, q = start;
            while (is_iter(q)) { ++niter; q += stride; }
            const double *pa[AMM_MAX_PRE] = {nullptr}, *pb[AMM_MAX_PRE] = {nullptr};
            double pc[AMM_MAX_PRE] = {0};
            int pp[AMM_MAX_PRE] = {0}, np = 0;
            double *f0 = slot(g->slot);
            if (bind_kicks(true, k, k + npre, pa, pb, pp, pc, np) && f0) {
                if (complete(f0) || complete_all(pa, pb, np)) return FAILED;
                ndef = 0;
                if (amm_inner_components_impl(ctx, bs, ctx->d_x, ctx->d_v, f0, np, pa, pb, pc, pp, ops[start].coef, ops[start + 1].coef,
                                              ops[start + eo + 1].coef, niter, bathed ? &ctx->baths[ops[start + 2].a] : nullptr,
                                              bathed ? ops[start + 3].coef : 0.0)) return FAILED;
                ctx->pos_epoch++;
                amm_watch_moved(ctx);
                k = q;
                return DONE;
            }
        }
        if (ndef) {
            // no component launch to ride on: the deferred kicks can still lead the launch of the run of plain kicks (+ move)
            // that opens this repetition (rule_kicks_move) -- a velocity-Verlet step is then KICK + KICK + MOVE in one
            int run = 0;
            while (is_kick(k + run)) ++run;
            if ((ctx->iso.on || ndef + run > 4) && flush_deferred()) return FAILED;
        }
        return NOT_MINE;
    }
    // 3. fused inner RESPA iteration: KICK(c1, fg) ; MOVE(d) ; EVAL(g) ; KICK(c2, fg) with g = one bond-list set
    // (kicks deferred from the previous repetition must not be overtaken by this block's move: deferral requires
    // f0_slot < 0, i.e. that this block never matched -- flushed here all the same, so that the order does not rest on that)
    // (regulated mode: k_fused_inner predicts the partners' positions with plain moves -- not taken)
    int rule_fused_inner(int &k) {
        const amm_op &op = ops[k];
        if (!(ctx->fuse_inner && !ctx->iso.on && !ctx->reg.on && op.op == AMM_OP_KICK && op.b < 0 && k + 3 < n_ops &&
              ops[k + 1].op == AMM_OP_MOVE && ops[k + 2].op == AMM_OP_EVAL)) return NOT_MINE;
        if (ndef && flush_deferred()) return FAILED;
        const GroupDef *g = ops[k + 3].op == AMM_OP_KICK && ops[k + 3].b < 0 && ops[k + 3].a == op.a ? group(ops[k + 2].a) : nullptr;
        BondedSet *bs = g && g->slot == op.a && (f0_slot < 0 || f0_slot == g->slot) ? sole_unsliced_bonded(*g) : nullptr;
        if (!bs) return NOT_MINE;
        if (!ctx->alt_x) {
            const size_t bytes = sizeof(double) * 3 * (size_t)ctx->n;
            AMM_HIP(hipMalloc(&ctx->alt_x, bytes));
            AMM_HIP(hipMalloc(&ctx->alt_v, bytes));
            AMM_HIP(hipMalloc(&ctx->alt_f, bytes));
        }
        if (f0_slot < 0) {
            f0_slot = g->slot;
            user_f0 = ctx->slots[f0_slot];
        }
        double *xi = ctx->d_x, *vi = ctx->d_v, *fi = ctx->slots[f0_slot];
        double *xo = swapped ? user_x : ctx->alt_x, *vo = swapped ? user_v : ctx->alt_v, *fo = swapped ? user_f0 : ctx->alt_f;
        if (amm_fused_inner_impl(ctx, bs, xi, vi, fi, xo, vo, fo, op.coef, ops[k + 1].coef, ops[k + 3].coef)) return FAILED;
        ctx->pos_epoch++;
        ctx->d_x = xo;
        ctx->d_v = vo;
        ctx->slots[f0_slot] = fo;
        ctx->slots[AMM_SLOT_X] = xo;
        ctx->slots[AMM_SLOT_V] = vo;
        swapped = !swapped;
        k += 4;
        return DONE;
    }
    // 4. EVAL(ga) ; EVAL(gb) of a guest pair force and the owner of its list, same positions: one pass for both
    int rule_dual_eval(int &k) {
        if (!(ctx->fuse_inner && ops[k].op == AMM_OP_EVAL && k + 1 < n_ops && ops[k + 1].op == AMM_OP_EVAL && ops[k].a != ops[k + 1].a))
            return NOT_MINE;
        const GroupDef *g1 = group(ops[k].a), *g2 = group(ops[k + 1].a);
        if (!g1 || !g2) return NOT_MINE;
        // further members of the two groups (bond-list terms, reciprocal space of a PME outer force) are added after
        // the shared pass; they must not be pair forces themselves
        auto tail_ok = [&](const GroupDef &g) {
            for (size_t j = 1; j < g.forces.size(); ++j)
                if (ctx->forces[g.forces[j]].type == AMM_FORCE_PAIR) return false;
            return true;
        };
        PairForce *pa = first_pair(*g1), *pb = first_pair(*g2);
        if (!(pa && pb && tail_ok(*g1) && tail_ok(*g2) && slot(g1->slot) && slot(g2->slot))) return NOT_MINE;
        PairForce *guest = pa->host == pb ? pa : (pb->host == pa ? pb : nullptr);
        if (!guest || g1->exchange != g2->exchange || !amm_pair_can_eval_dual(ctx, guest, guest->host)) return NOT_MINE;
        double *fg = ctx->slots[guest == pa ? g1->slot : g2->slot], *fh = ctx->slots[guest == pa ? g2->slot : g1->slot];
        // the kicks and the inner loop that follow as the launch's epilogue, when both groups are the pair forces alone
        EpiPlan plan;
        int q_resume = 0;
        bool wraps = false;
        // (several ranks: only groups whose exchange is the all-gather of slices -- the launch then integrates
        // this rank's molecules and the ranks exchange positions and velocities: cluster.hip, state exchange)
        const bool planned = (ctx->world == 1 ? !g1->exchange : g1->exchange == AMM_EXCHANGE_GATHER) && g1->forces.size() == 1 &&
                             g2->forces.size() == 1 && plan_epilogue(k + 2, plan, q_resume, wraps);
        ctx->epi_request = planned ? &plan : nullptr;
        ctx->epi_done = false;
        if (planned) ctx->n_plan_offers++;
        const int rc_dual = amm_pair_eval_impl(ctx, guest->host, ctx->d_x, fh, 0, nullptr, guest, fg, 0, g1->exchange);
        ctx->epi_request = nullptr;
        if (rc_dual) return FAILED;
        // (a yield here: further members of the two groups are added after the exchange: only pair-only groups get there --
        // an exchanged group holds exactly one pair force)
        if (const int r = after_planned_eval(k, q_resume, wraps, k + 2, fh, fg); r != NOT_MINE) return r;
        for (const GroupDef *g : {g1, g2})
            for (size_t j = 1; j < g->forces.size(); ++j)
                if (amm_force_eval_dispatch(ctx, g->forces[j], ctx->d_x, ctx->slots[g->slot], 1, nullptr)) return FAILED;
        k += 2;
        return DONE;
    }
    // 5. EVAL(g) ; KICK ... [; MOVE] with g = a term-parallel bond-list set [+ an interaction-group pair force with a small set,
    // which group.hip evaluates without a list and which writes EVERY row]: the pair force goes first, the terms are
    // evaluated, and the launch that gathers their forces also applies the kicks and the move that follow -- an inner RESPA
    // iteration of a system that is not pure water (config C5: chain + solute + waters) is then 3 launches, not 8.
    // (regulated mode: the gather launch's move is a plain one -- not taken)
    int rule_terms_kicks(int &k) {
        const GroupDef *g = ops[k].op == AMM_OP_EVAL ? group(ops[k].a) : nullptr;
        if (!(ctx->fuse_inner && !ctx->iso.on && !ctx->reg.on && g && g->slot >= 0 && !g->exchange && is_kick(k + 1))) return NOT_MINE;
        BondedSet *bs = nullptr;
        PairForce *ps = nullptr;
        bool plain = g->forces.size() >= 1 && g->forces.size() <= 2;
        for (int fid : g->forces) {
            const ForceObj &fo = ctx->forces[fid];
            PairForce *pf = fo.pair();
            if (fo.bonded() && !bs) bs = fo.bonded();
            else if (pf && !ps && pf->small && ctx->opt_small_group && !pf->built && amm_small_group_supported(pf)) ps = pf;
            else plain = false;
        }
        double *buf = ctx->slots[g->slot];
        if (!(plain && bs && buf && bs->n_gterms > 0 && !(bs->sliced && ctx->world > 1) && ctx->world == 1)) return NOT_MINE;
        KickList K = {};
        int j = k + 1;
        while (is_kick(j) && j - (k + 1) < 4) ++j;
        if (!bind_kicks(false, k + 1, j, K.f, K.f2, K.plus, K.coef, K.n)) return NOT_MINE;
        const bool more_kicks = is_kick(j);      // a fifth kick: left to the next launch
        const bool moves = !more_kicks && j < n_ops && ops[j].op == AMM_OP_MOVE;
        // (the pair force's launch evaluates the bond-list terms too: group.hip, TermsWork)
        const double *pair_rows = nullptr;         // (the pair force's rows: in `buf`, or in a buffer of its own)
        const bool own = bs->mixed_ok && ctx->opt_mixed_terms;       // (k_mixed_eval_kicks takes them from anywhere)
        if (ps && amm_small_group_eval_impl(ctx, ps, ctx->d_x, buf, 0, nullptr, bs, own ? &pair_rows : nullptr) != 0) return FAILED;
        if (amm_bonded_eval_kicks_impl(ctx, bs, ctx->d_x, buf, ps ? 1 : 0, K, moves ? 1 : 0, moves ? ops[j].coef : 0.0, ps ? 1 : 0, pair_rows)) return FAILED;
        if (moves) {
            ctx->pos_epoch++;
            amm_watch_moved(ctx);
        }
        k = j + (moves ? 1 : 0);
        return DONE;
    }
    // 6. a run of plain kicks, then (maybe) a move: one launch (same arithmetic per degree of freedom, same order)
    int rule_kicks_move(int &k) {
        if (!(ctx->fuse_inner && !ctx->iso.on && ops[k].op == AMM_OP_KICK)) return NOT_MINE;
        const double *fa[4], *fb[4];
        int plus[4], nk = 0;
        double coef[4];
        // (kicks deferred from the end of the previous repetition come first: the order they were written in)
        if (ndef && !bind_kicks(true, k, k, fa, fb, plus, coef, nk)) {
            if (flush_deferred()) return FAILED;         // (reports the unbound buffer)
            nk = 0;
        }
        const int nlead = nk;
        int j = k;
        while (is_kick(j) && nlead + (j - k) < 4) ++j;
        bind_kicks(false, k, j, fa, fb, plus, coef, nk);        // (stops at an unbound buffer: left to the plain path, which reports it)
        j = k + (nk - nlead);
        const bool moves = j < n_ops && ops[j].op == AMM_OP_MOVE;
        const bool whole_run = !is_kick(j);       // (a fifth kick: the run goes on)
        if ((nlead == 0 || whole_run) && (nk >= 2 || (nk == 1 && moves))) {
            if (complete_all(fa, fb, nk)) return FAILED;
            if (amm_kicks_move_impl(ctx, fa, fb, plus, coef, nk, moves ? 1 : 0, moves ? ops[j].coef : 0.0)) return FAILED;
            ndef = 0;
            if (moves) {
                ctx->pos_epoch++;
                amm_watch_moved(ctx);
            }
            k = j + (moves ? 1 : 0);
            return DONE;
        }
        if (ndef && flush_deferred()) return FAILED;       // (not taken along: before anything else, in their order)
        return NOT_MINE;
    }

    // ---- 7. the plain ops ----
    // EVAL of a group that is one pair force with a list: the kicks and the inner loop that follow can ride on its launch (molecule
    // rows: cepi_rows; several ranks: followed by an exchange of positions and velocities instead of forces)
    int eval_planned(int &k, const GroupDef &g, double *buf) {
        PairForce *pf = (ctx->world == 1 ? !g.exchange : g.exchange == AMM_EXCHANGE_GATHER) ? sole_listed_pair(g) : nullptr;
        EpiPlan plan;
        int q_resume = 0;
        bool wraps = false;
        if (!pf || !(plan_epilogue(k + 1, plan, q_resume, wraps) ||
                     (pf->all_q_zero && !pf->cluster_ok && plan_atoms(k + 1, plan, q_resume, wraps)))) return NOT_MINE;
        ctx->epi_request = &plan;
        ctx->epi_done = false;
        ctx->n_plan_offers++;
        const int rc_one = amm_pair_eval_impl(ctx, pf, ctx->d_x, buf, 0, nullptr, nullptr, nullptr, 0, g.exchange);
        ctx->epi_request = nullptr;
        if (rc_one) return FAILED;
        const int r = after_planned_eval(k, q_resume, wraps, k + 1, buf, nullptr);
        if (r == NOT_MINE) k += 1;          // (no epilogue: the evaluation alone)
        return r == NOT_MINE ? DONE : r;
    }
    int run_eval(int &k) {
        const GroupDef *gp = group(ops[k].a);
        if (!gp || gp->slot < 0) {
            amm_set_error("amm_run_ops: EVAL of an undefined group");
            return FAILED;
        }
        const GroupDef &g = *gp;
        double *buf = ctx->slots[g.slot];
        if (!buf) {
            amm_set_error("amm_run_ops: group buffer not bound");
            return FAILED;
        }
        if (g.forces.empty()) AMM_HIP(hipMemsetAsync(buf, 0, sizeof(double) * 3 * (size_t)ctx->n, ctx->stream));
        if (const int r = eval_planned(k, g, buf); r != NOT_MINE) return r;
        forget_own_only(buf);           // (every path below writes the group's buffer in full)
        ++k;
        if (g.exchange) {
            PairForce *pf = sole_listed_pair(g);
            if (!pf) {
                amm_set_error("amm_run_ops: an exchanged group must hold exactly one pair force (with a neighbour list)");
                return FAILED;
            }
            if (amm_pair_eval_impl(ctx, pf, ctx->d_x, buf, 0, nullptr, nullptr, nullptr, 0, 1)) return FAILED;
            return leave_to_host(pos(rep, k));
        }
        // FarNonbondedForce (forces.py:710-724) = total + discount, two forces of one group: when the discount
        // (guarded near force, sign -1) shares the total's neighbour list, both are evaluated in ONE traversal that
        // accumulates into the same buffer (the reference, and OpenMM, run two passes)
        const size_t nf = g.forces.size();
        auto pair_of = [&](size_t i) { return ctx->forces[g.forces[i]].pair(); };
        std::vector<char> done(nf, 0);
        bool first = true;
        for (size_t j = 0; j < nf; ++j) {
            if (done[j]) continue;
            if (PairForce *pj = pair_of(j)) {
                size_t partner = nf;
                for (size_t i = 0; i < nf && partner == nf; ++i)
                    if (i != j && !done[i] && pair_of(i) && amm_pair_can_fuse_discount(ctx, pair_of(i), pj)) partner = i;
                if (partner < nf) {
                    if (amm_pair_eval_impl(ctx, pj, ctx->d_x, buf, first ? 0 : 1, nullptr, pair_of(partner), buf, 1, 0)) return FAILED;
                    done[j] = done[partner] = 1;
                    first = false;
                    continue;
                }
                // the discount itself comes later in the list: let its host pick it up
                bool is_discount = false;
                for (size_t i = 0; i < nf; ++i)
                    if (i != j && !done[i] && pair_of(i) && amm_pair_can_fuse_discount(ctx, pj, pair_of(i))) is_discount = true;
                if (is_discount) continue;
            }
            if (amm_force_eval_dispatch(ctx, g.forces[j], ctx->d_x, buf, first ? 0 : 1, nullptr)) return FAILED;
            done[j] = 1;
            first = false;
        }
        for (size_t j = 0; j < nf; ++j)      // (a discount whose host was consumed by another pairing)
            if (!done[j]) {
                if (amm_force_eval_dispatch(ctx, g.forces[j], ctx->d_x, buf, first ? 0 : 1, nullptr)) return FAILED;
                first = false;
            }
        return DONE;
    }
    int run_plain(int &k) {
        const amm_op &op = ops[k];
        if (op.op == AMM_OP_EVAL) {
            // (with virtual sites: what the sites collected goes to their parents as soon as the group's buffer is full)
            const int r = run_eval(k);
            if (r != DONE || !ctx->vsites) return r;
            return amm_vsite_spread_impl(ctx, ctx->d_x, ctx->slots[ctx->groups[op.a].slot]) ? FAILED : DONE;
        }
        switch (op.op) {
        case AMM_OP_KICK: {
            const double *fa, *fb;
            int plus, n = 0;
            double coef;
            if (!bind_kicks(false, k, k + 1, &fa, &fb, &plus, &coef, n)) {
                amm_set_error("amm_run_ops: KICK buffer not bound");
                return FAILED;
            }
            if (complete(fa) || complete(fb)) return FAILED;
            if (amm_kick_impl(ctx, ctx->d_v, fa, fb, plus, ctx->d_mass, coef)) return FAILED;
        } break;
        case AMM_OP_MOVE:
            if (amm_move_impl(ctx, ctx->d_x, ctx->d_v, op.coef)) return FAILED;
            if (x_written()) return FAILED;
            break;
        case AMM_OP_COPY:
            if (copy_op(op, true)) return FAILED;
            if (slot(op.a) == ctx->d_x && x_written()) return FAILED;
            break;
        case AMM_OP_COMBINE: {
            double *dst = slot(op.a), *sa = slot(op.b), *sb = slot(op.c);
            if (!dst || !sa || !sb) {
                amm_set_error("amm_run_ops: COMBINE buffer not bound");
                return FAILED;
            }
            if (complete(sa) || complete(sb)) return FAILED;
            if (amm_combine_impl(ctx, dst, sa, sb, op.coef)) return FAILED;
            if (dst == ctx->d_x && x_written()) return FAILED;
        } break;
        case AMM_OP_EXPR: {
            double *dst = slot(op.b);
            if (op.a < 0 || op.a >= (int)ctx->exprs.size() || !dst) {
                amm_set_error("amm_run_ops: EXPR with an unknown expression or an unbound destination");
                return FAILED;
            }
            const ExprDef &e = ctx->exprs[op.a];
            // the high bit of the counter keeps these streams apart from those of direct amm_expr_eval calls.  An expression whose
            // code draws no random number takes no counter: a step's random ops then see the same counters whatever deterministic
            // expressions stand between them (a stock integrator's op-by-op step draws what its AMM_OP_STOCK draws)
            bool draws = false;
            for (const int32_t word : e.code) draws = draws || (word & 0xFF) == X_GAUSS || (word & 0xFF) == X_UNIFORM;
            const unsigned long long counter = (1ull << 63) | (draws ? ++ctx->expr_counter : ctx->expr_counter);
            if (amm_expr_eval_impl(ctx, e.code.data(), (int)e.code.size(), e.consts.data(), (int)e.consts.size(),
                                   e.globals.data(), (int)e.globals.size(), ctx->expr_seed, counter, dst, nullptr)) return FAILED;
        } break;
        case AMM_OP_SAVE_REF:
        case AMM_OP_CONSTRAIN_X:
        case AMM_OP_CONSTRAIN_V: {
            if (!ctx->constraints) break;       // no constraints in the System: identity (OpenMM does the same)
            if (op.op == AMM_OP_SAVE_REF) {
                if (amm_constraints_save_reference(ctx, ctx->constraints, ctx->d_x)) return FAILED;
            } else if (op.op == AMM_OP_CONSTRAIN_X) {
                if (amm_constrain_positions(ctx, ctx->constraints, ctx->d_x)) return FAILED;
                if (x_written()) return FAILED;
            } else if (amm_constrain_velocities(ctx, ctx->constraints, ctx->d_x, ctx->d_v)) return FAILED;
        } break;
        case AMM_OP_BATH: {
            if (op.a < 0 || op.a >= (int)ctx->baths.size()) {
                amm_set_error("amm_run_ops: BATH with an unknown bath id");
                return FAILED;
            }
            if (amm_bath_impl(ctx, ctx->baths[op.a], ctx->d_v, (1ull << 63) | ++ctx->expr_counter)) return FAILED;
        } break;
        case AMM_OP_STOCK: {
            const double *f = slot(op.b);
            if (op.a < 0 || op.a >= (int)ctx->stocks.size()) {
                amm_set_error("amm_run_ops: STOCK with an unknown stock id");
                return FAILED;
            }
            if (!f) {
                amm_set_error("amm_run_ops: STOCK force buffer not bound");
                return FAILED;
            }
            if (ctx->iso.on || ctx->reg.on) {
                amm_set_error("amm_run_ops: STOCK does not run in the isokinetic or the regulated mode");
                return FAILED;
            }
            if (complete(f)) return FAILED;
            if (amm_stock_step_impl(ctx, ctx->stocks[op.a], f, (1ull << 63) | ++ctx->expr_counter)) return FAILED;
            if (x_written()) return FAILED;
            // (the launch evaluated the lists' displacement triggers -- for the atoms it moved, not for sites placed since)
            if (!ctx->vsites) amm_watch_moved(ctx);
        } break;
        case AMM_OP_DRUDE_STEP: {
            const double *f = slot(op.b);
            if (op.a < 0 || op.a >= (int)ctx->drude_steps.size()) {
                amm_set_error("amm_run_ops: DRUDE_STEP with an unknown step id");
                return FAILED;
            }
            if (!f) {
                amm_set_error("amm_run_ops: DRUDE_STEP force buffer not bound");
                return FAILED;
            }
            if (ctx->iso.on || ctx->reg.on) {
                amm_set_error("amm_run_ops: DRUDE_STEP does not run in the isokinetic or the regulated mode");
                return FAILED;
            }
            if (complete(f)) return FAILED;
            if (amm_drude_step_impl(ctx, ctx->drude_steps[op.a], f, (1ull << 63) | ++ctx->expr_counter)) return FAILED;
            if (x_written()) return FAILED;
            if (!ctx->vsites) amm_watch_moved(ctx);
        } break;
        case AMM_OP_ALLREDUCE: {
            if (!slot(op.a)) {
                amm_set_error("amm_run_ops: ALLREDUCE of an unbound buffer");
                return FAILED;
            }
            // consecutive all-reduces of buffers that are neighbours in memory (the near and the outer force after a
            // dual evaluation) travel as ONE message: the exchange is latency bound at 2.4 MB
            const size_t n3 = 3 * (size_t)ctx->n;
            double *lo = slot(op.a);
            size_t count = n3;
            while (k + 1 < n_ops && ops[k + 1].op == AMM_OP_ALLREDUCE && slot(ops[k + 1].a)) {
                double *nb = slot(ops[k + 1].a);
                if (nb == lo + count) count += n3;
                else if (nb + n3 == lo) { lo = nb; count += n3; }
                else break;
                ++k;
            }
            if (amm_comm_allreduce_impl(ctx, lo, count)) return FAILED;
        } break;
        default: amm_set_error("amm_run_ops: unknown op"); return FAILED;
        }
        ++k;
        return DONE;
    }

    // One scheduling decision at op k.  The rules are tried in this order, and the order is their priority:
    //   1 first: once 2 or 6 has launched the kicks that close the repetition there is nothing left to defer.
    //   2 before 3: all inner iterations and the kicks in front of them in ONE launch beats one launch per iteration; 3 is what is left
    //     for sets whose components are too large for 2.  2 also decides what becomes of deferred kicks it could not take along (kept
    //     for 6, or flushed).
    //   3 flushes the deferred kicks first: its move must not overtake them.  3 before 6: 6 would take the iteration's KICK + MOVE.
    //   4 and 5 start at an EVAL and differ in the op behind it (an EVAL / a KICK): their order is free.  Both before 7, which would
    //     walk the list twice / launch the kicks on their own; 5 before 6 in effect, as it consumes the kicks 6 would take.
    //   6 before 7: a run of kicks [+ move] is one launch; 6 is the last taker of deferred kicks and flushes those it leaves.
    //   7 runs the op alone, and reports what is wrong with it.
    // (Deferred kicks reach 2, 3 and 6 only: anything but a KICK at op 0 flushes them first.)
    int step(int &k) {
        if (ndef && !(k == 0 && ops[k].op == AMM_OP_KICK) && flush_deferred()) return FAILED;
        // virtual sites: every position update is followed by a placement and every evaluation by a spread, which no fused launch
        // does -- every op runs on its own (the near force riding on the outer force's traversal inside run_eval fills the same
        // buffer and stays)
        if (ctx->vsites) return taken(0, run_plain(k));
        int r;
        if ((r = rule_defer_trailing_kicks(k)) != NOT_MINE) return taken(1, r);
        if ((r = rule_inner_components(k)) != NOT_MINE) return taken(2, r);
        if ((r = rule_fused_inner(k)) != NOT_MINE) return taken(3, r);
        if ((r = rule_dual_eval(k)) != NOT_MINE) return taken(4, r);
        if ((r = rule_terms_kicks(k)) != NOT_MINE) return taken(5, r);
        if ((r = rule_kicks_move(k)) != NOT_MINE) return taken(6, r);
        return taken(0, run_plain(k));
    }
    // statistics (amm_run_rule_stats): who made the decision that run() counts in n_sched
    int taken(int rule, int r) {
        if (r != FAILED) ctx->n_rule[rule]++;
        return r;
    }
    int run() {
        k_start = cursor ? (int)(*cursor % n_ops) : 0;
        for (rep = cursor ? (int)(*cursor / n_ops) : 0; rep < repeat && !yielded; ++rep) {
            int k = k_start;
            k_start = 0;
            while (k < n_ops && !yielded) {
                const int r = step(k);
                if (r == FAILED) return 1;
                ctx->n_sched++;
                yielded = r == YIELDED;
            }
        }
        if (flush_deferred()) return 1;
        if (cursor && !yielded) *cursor = total_ops;
        if (!yielded && !ctx->own_only.empty()) {
            // the program is through: the caller may read any force buffer now (the engine serves cached forces): bond-list groups are
            // evaluated again in full, a pair group left with this rank's rows only is an error (a RESPA program ends on a whole evaluation)
            const std::vector<const double *> left = ctx->own_only;
            for (const double *b : left)
                if (complete(b)) return 1;
        }
        if (swapped) {   // odd number of fused iterations: bring the state back into the caller's buffers
            const size_t bytes = sizeof(double) * 3 * (size_t)ctx->n;
            AMM_HIP(hipMemcpyAsync(user_x, ctx->d_x, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            AMM_HIP(hipMemcpyAsync(user_v, ctx->d_v, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            AMM_HIP(hipMemcpyAsync(user_f0, ctx->slots[f0_slot], bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        restore(false);        // the copies above were checked; only the pointers are left to rebind
        return 0;
    }
};

}  // namespace

// the caller (abi.hip) has validated ctx and ops, and n_ops > 0, repeat > 0
int amm_run_ops_impl(amm_ctx *ctx, const amm_op *ops, int n_ops, int repeat, int64_t *cursor) {
    if (!ctx->d_x || !ctx->d_v || !ctx->d_mass) {
        amm_set_error("amm_run_ops: state not bound (amm_bind_state)");
        return 1;
    }
    if (cursor && (*cursor < 0 || *cursor > (long)repeat * n_ops)) {
        amm_set_error("amm_run_ops_from: cursor out of range");
        return 1;
    }
    // (*cursor == total_ops: nothing left to run -- the call winds the program up: force buffers that hold this rank's rows only)
    if (ctx->pending.active) {
        amm_set_error("amm_run_ops: an exchanged evaluation still waits for amm_exchange_finish");
        return 1;
    }
    if (!ctx->opt_positions_private) ctx->pos_epoch++;                 // the caller may have written the bound position buffer
    return OpRun(ctx, ops, n_ops, repeat, cursor).run();
}
