// dpg_chol.hip -- driver of the supernodal multifrontal Cholesky of the pose-graph normal equations
// on gfx950: the CHOLESKY solve that GTSAM runs inside GaussNewtonOptimizer / ISAM2.
// The symbolic analysis (dpg_chol_sym.cpp) and the host planner that builds every index table the
// kernels follow (dpg_chol_plan.cpp, plain C++) run once per sparsity pattern; this file creates
// the solver object, uploads the plan and holds the solve entry points (full, partial, gated,
// resolve).  The kernels with their launch helpers are in dpg_chol_level / _factor / _solve / _sel
// .hip (dpg_chol_dev.h).  The fronts of one factorization stay resident in HBM (tens of MB).
#include "dpg_chol_dev.h"

using namespace dpg_chol;

namespace {
// a new analysis in; *S gets back one whose buffers the caller reuses.  With tracking, the analysis
// of the last factorization moves to fac_sym instead (the partial refactorization compares with it)
void take_sym(CholDev* c, dpg_chol_sym* S) {
    c->has_factor = false;   // (the values in fronts belong to the analysis leaving)
    if (c->track && c->sym_is_fac) {
        std::swap(c->fac_sym, c->sym);
        c->fac_G.swap(c->plan.cur_G);
        c->sym_is_fac = false;
    }
    std::swap(c->sym, *S);
}

// The structure arrays are packed into one pinned staging buffer and go up in ONE asynchronous
// copy into one device arena (the pointers of c point into it); one synchronisation at the end.
int chol_upload(CholDev* c) {
    const dpg_chol_sym& S = c->sym;
    const CholPlan& H = c->plan;
    const int64_t n = H.n;
    ++c->build_gen;   // (the selected inverse's lists follow the analysis: rebuilt on its next request)
    c->has_factor = false;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    struct Piece { void** d; const void* h; size_t bytes; };
    Piece pieces[24];
    int np = 0;
    auto add = [&](auto** d, const auto& h) {
        using T = typename std::remove_reference<decltype(h)>::type::value_type;
        pieces[np++] = Piece{reinterpret_cast<void**>(d), h.data(), h.size() * sizeof(T)};
    };
    add(&c->sns, H.sns);
    add(&c->omap, H.omap);
    add(&c->child_list, S.child_list);
    add(&c->relmap, S.relmap);
    add(&c->rows, S.sn_rows);
    add(&c->perm, S.perm);
    add(&c->pos, S.pos);
    add(&c->order_fwd, H.fo);
    add(&c->order_fac, H.order_fac);
    add(&c->ftasks, H.ftasks);
    add(&c->fchild, H.fchild);
    add(&c->order_bwd, H.bwd);
    add(&c->segs, H.segs);
    add(&c->dblocks, H.dblocks);
    add(&c->inv_tasks, H.inv_t);
    if (!H.fused) {
        add(&c->asm_tasks, H.asm_t);
        add(&c->asm_child, H.asm_c);
        add(&c->panel_tasks, H.panel_t);
        add(&c->upd_tasks, H.upd_t);
    }
    size_t total = 0;
    for (int i = 0; i < np; ++i) total += al(std::max<size_t>(pieces[i].bytes, 1));
    if (c->stage.reserve_amortised(total) || c->arena.reserve_amortised(total)) return DPG_ERR_HIP;
    size_t off = 0;
    for (int i = 0; i < np; ++i) {
        if (pieces[i].bytes) memcpy(c->stage.p + off, pieces[i].h, pieces[i].bytes);
        *pieces[i].d = c->arena.p + off;
        off += al(std::max<size_t>(pieces[i].bytes, 1));
    }
    int rc = hipMemcpyAsync(c->arena.p, c->stage.p, total, hipMemcpyHostToDevice, nullptr) != hipSuccess;
    // a re-allocated front, y or pending-update buffer has lost the tracked factorization (a new
    // allocation may come back at the old address: the capacities tell)
    const size_t cap0[3] = {c->fronts.cap, c->acc.cap, c->ysol.cap};
    rc |= c->sync.reserve_amortised(H.sync_bytes / sizeof(int32_t));
    rc |= c->fronts.reserve_amortised((size_t)S.front_off[(size_t)S.ns]);
    rc |= c->acc.reserve_amortised((size_t)H.acc_total);
    rc |= c->ysol.reserve_amortised((size_t)(3 * n));
    if (rc || cap0[0] != c->fronts.cap || cap0[1] != c->acc.cap || cap0[2] != c->ysol.cap) c->fac_valid = false;
    rc |= c->xsol.reserve_amortised((size_t)(3 * n));
    rc |= c->status.reserve_amortised(1);
    rc |= c->dinv.reserve_amortised((size_t)(3 * n) * kSB);
    rc |= c->linv.reserve_amortised((size_t)std::max<int64_t>(H.linv_total, 1));
    if (!rc) rc |= hipMemsetAsync(c->status.p, 0, sizeof(int32_t), nullptr) != hipSuccess;
    // the staging buffer is reused by the next build: wait for the copy (always, even after an error)
    rc |= hipStreamSynchronize(nullptr) != hipSuccess;
    return rc ? DPG_ERR_HIP : DPG_OK;
}

// (a plan and its upload may be split: dpg_chol_create_sym_plan / _upload, possibly on two threads
// one after the other)
int chol_build_plan(CholDev* c, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs) {
    const double t_b0 = now_ms();
    const int rc = dpg_chol_plan_build(c->plan, c->sym, c->opts, c->track, n, pair_lo, pair_hi, n_pairs);
    c->t_build[0] = now_ms() - t_b0;
    return rc;
}
int chol_build_upload(CholDev* c) {
    const double t_b1 = now_ms();
    const int rc = chol_upload(c);
    c->t_build[1] = now_ms() - t_b1;
    return rc;
}
int chol_build(CholDev* c, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs) {
    const int rc = chol_build_plan(c, n, pair_lo, pair_hi, n_pairs);
    return rc ? rc : chol_build_upload(c);
}

// reuse *h or create the object, take the options, take the analysis (*S gets an earlier one: its
// buffers are reused by the next derive)
CholDev* chol_take(void** h, dpg_chol_sym* S, const dpg_chol_opts* opts) {
    CholDev* c = *h ? reinterpret_cast<CholDev*>(*h) : new CholDev();
    if (opts) c->opts = *opts;
    take_sym(c, S);
    return c;
}
// the end of a build step of c: *h = c, or on an error c destroyed and *h = NULL
int chol_built(void** h, CholDev* c, int rc) {
    if (rc) dpg_chol_destroy(c);
    *h = rc ? nullptr : c;
    return rc;
}
}  // namespace

extern "C" void dpg_chol_destroy(void* h) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c) return;
    if (c->aux.s) (void)hipStreamSynchronize(c->aux.s);
    delete c;
}

extern "C" int dpg_chol_create(void** out, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi,
                               int64_t n_pairs, const dpg_chol_opts* opts) {
    *out = nullptr;
    CholDev* c = new CholDev();
    if (opts) c->opts = *opts;
    if (dpg_chol_symbolic(n, pair_lo, pair_hi, n_pairs, &c->opts, &c->sym)) {
        delete c;
        return DPG_ERR_NUMERIC;
    }
    return chol_built(out, c, chol_build(c, n, pair_lo, pair_hi, n_pairs));
}

// The same from a given symbolic analysis; *h is reused (its buffers grow when needed) or created.
int dpg_chol_create_sym(void** h, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs,
                        dpg_chol_sym* S, const dpg_chol_opts* opts) {
    CholDev* c = chol_take(h, S, opts);
    return chol_built(h, c, chol_build(c, n, pair_lo, pair_hi, n_pairs));
}

// dpg_chol_create_sym in two halves: the plan (host only: no device call, so it may run while the
// caller's stream still works, on any thread) and the upload of what it planned (nothing between)
int dpg_chol_create_sym_plan(void** h, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs,
                             dpg_chol_sym* S, const dpg_chol_opts* opts) {
    CholDev* c = chol_take(h, S, opts);
    return chol_built(h, c, chol_build_plan(c, n, pair_lo, pair_hi, n_pairs));
}
int dpg_chol_create_sym_upload(void** h) {
    CholDev* c = reinterpret_cast<CholDev*>(*h);
    return c ? chol_built(h, c, chol_build_upload(c)) : DPG_ERR_STATE;
}
// the plan's first stage ahead of the plan (pos / perm: the ordering the plan's analysis will
// carry); creates the solver object when *h is NULL.  Host only; not concurrently with a plan or an
// upload of the same object.
int dpg_chol_plan_blocks(void** h, int64_t n, const int32_t* pos, const int32_t* perm, const int32_t* pair_lo,
                         const int32_t* pair_hi, int64_t n_pairs) {
    if (!h || n <= 0 || !pos || !perm || n_pairs < 0 || (n_pairs > 0 && (!pair_lo || !pair_hi))) return DPG_ERR_ARG;
    CholDev* c = *h ? reinterpret_cast<CholDev*>(*h) : new CholDev();
    *h = c;
    dpg_chol_plan_prebucket(c->plan, n, pos, perm, pair_lo, pair_hi, n_pairs);
    return DPG_OK;
}
// drop prebuilt H-block buckets (their ordering was not the one the next plan will carry: the
// derivation they were built beside failed)
void dpg_chol_blocks_invalidate(void* h) {
    if (h) reinterpret_cast<CholDev*>(h)->plan.blocks_ready = false;
}
int dpg_chol_fused(void* h) { return h && reinterpret_cast<const CholDev*>(h)->plan.fused ? 1 : 0; }

void dpg_chol_build_times(void* h, double out[2]) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    out[0] = c ? c->t_build[0] : 0.0;
    out[1] = c ? c->t_build[1] : 0.0;
}

// the values in fronts now belong to the current analysis
static void note_factored(CholDev* c, int64_t refactored, int64_t kept, int64_t moved, int64_t pick_ns = 0) {
    c->pstats[0] = refactored;
    c->pstats[1] = kept;
    c->pstats[2] = moved;
    c->pstats[3] = pick_ns;
    c->has_factor = true;
    if (!c->track) return;
    c->fac_valid = true;
    c->fac_ptr = c->fronts.p;
    c->fac_ysol = c->ysol.p;
    c->fac_acc = c->acc.p;
    c->sym_is_fac = true;
    c->fac_db = c->plan.fused_db;
}

extern "C" int dpg_chol_solve(void* h, const double* hb, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    const CholPlan& P = c->plan;
    note_factored(c, c->sym.ns, 0, 0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess) return DPG_ERR_HIP;
    if (P.fused) {
        if (hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
        launch_factor(c, st, hb, nullptr, nullptr);
    } else {
        launch_levels(c, st, hb);
        if (hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
    }
    const double* di = launch_inv_diag(c, st);
    if (!P.fused) launch_forward(c, st, hb, di, nullptr, nullptr);
    launch_backward(c, st, di, nullptr, nullptr, nullptr, nullptr);
    // the inverse after the backward (which, as a refactoring iteration of the gated loop, chains):
    // the chord steps of dpg_chol_resolve then do the same arithmetic as the gated loop's
    c->inv_valid = c->keep_inv && P.n_inv_tasks > 0;
    if (c->inv_valid) launch_inv(c, st, nullptr);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

extern "C" void dpg_chol_track_factor(void* h, int on) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c || c->track == (on != 0)) return;
    c->track = on != 0;
    c->fac_valid = false;
    c->sym_is_fac = false;
    c->plan.cur_G.clear();   // the current analysis was planned untracked: its team sizes are unknown
}
extern "C" void dpg_chol_forget_factor(void* h) {
    if (!h) return;
    reinterpret_cast<CholDev*>(h)->fac_valid = false;
    reinterpret_cast<CholDev*>(h)->has_factor = false;
}
extern "C" void dpg_chol_partial_stats(void* h, int64_t out[4]) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    for (int k = 0; k < 4; ++k) out[k] = c ? c->pstats[k] : 0;
}

// ISAM2's partial re-elimination (isam_->update, dpg_slam.cc:320, re-eliminates only the cliques
// the new factors touch and their ancestors), as a multifrontal refactorization that keeps every
// front whose values cannot have changed since the tracked factorization (the rule:
// dpg_chol_plan_partial; here: the old order is a prefix of the new, the same panel buffering).
// The forward solve folded into the factorization keeps its values too: a kept front's nodes have
// the same gradient (no new factor on them, same theta) and its children are kept, so its part of y
// (at its column positions: unchanged between reorders) and its pending row updates for the parent
// are what a full refactorization would compute again.  A kept front the new layout moved -- its
// values and its pending updates -- goes through the scratch buffer (gather, scatter), then the
// factorization runs with the kept fronts only signalling their parents, then the backward solve
// over every front.  The result is bit-identical to dpg_chol_solve's.
extern "C" int dpg_chol_solve_partial(void* h, const double* hb, const int32_t* dirty_nodes, int64_t n_dirty,
                                      void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    const dpg_chol_sym& S = c->sym;
    const dpg_chol_sym& O = c->fac_sym;
    const CholPlan& P = c->plan;
    const bool usable = c->track && c->fac_valid && !c->sym_is_fac && c->fac_ptr == c->fronts.p &&
                        c->fac_ysol == c->ysol.p && c->fac_acc == c->acc.p && P.fused &&
                        !(P.use_dinv && P.n_dblocks > 0) && c->fac_db == P.fused_db && O.ns > 0 && O.n <= S.n &&
                        (int64_t)c->fac_G.size() == (int64_t)O.ns && (int64_t)P.cur_G.size() == (int64_t)S.ns &&
                        std::equal(O.perm.begin(), O.perm.end(), S.perm.begin());
    // the pick (dpg_chol_plan.cpp): the kept fronts and the runs that move them, or refactor everything
    const double t_pick = now_ms();
    PartialPick& K = c->pick;
    if (!usable || !dpg_chol_plan_partial(K, S, O, P.cur_G, c->fac_G, dirty_nodes, n_dirty)) return dpg_chol_solve(h, hb, stream);
    const int32_t ns = S.ns;
    const int64_t nruns = (int64_t)K.runs.size() / 4;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // keep flags + gather runs + scatter runs: one pinned buffer, one copy up
    const size_t keep_bytes = ((size_t)ns + 15) & ~size_t(15);
    const size_t run_bytes = sizeof(int64_t) * 4 * (size_t)nruns;
    const size_t bytes = keep_bytes + 2 * run_bytes;
    if (c->pev_set && hipEventSynchronize(c->pev.e) != hipSuccess) return DPG_ERR_HIP;
    if (c->pstage.reserve_amortised(bytes) || c->dpart.reserve_amortised(bytes) ||
        (K.moved > 0 && c->scratch.reserve_amortised((size_t)K.moved)))
        return DPG_ERR_HIP;
    memcpy(c->pstage.p, K.keep.data(), (size_t)ns);
    int64_t* gat = reinterpret_cast<int64_t*>(c->pstage.p + keep_bytes);
    int64_t* sca = gat + 4 * nruns;
    for (int64_t r = 0, off = 0; r < nruns; ++r) {
        const int64_t* q = K.runs.data() + 4 * r;
        const int64_t g4[4] = {q[0], off, q[2], q[3]}, s4[4] = {off, q[1], q[2], q[3]};
        std::copy(g4, g4 + 4, gat + 4 * r);
        std::copy(s4, s4 + 4, sca + 4 * r);
        off += q[2];
    }
    if (c->pev.ensure(hipEventDisableTiming)) return DPG_ERR_HIP;
    if (hipMemcpyAsync(c->dpart.p, c->pstage.p, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(c->pev.e, st) != hipSuccess)
        return DPG_ERR_HIP;
    c->pev_set = true;
    const uint8_t* keep_dev = reinterpret_cast<const uint8_t*>(c->dpart.p);
    const int64_t* gat_dev = reinterpret_cast<const int64_t*>(c->dpart.p + keep_bytes);
    launch_copy_runs(c, st, gat_dev, gat_dev + 4 * nruns, nruns, K.max_run);
    if (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess)
        return DPG_ERR_HIP;
    launch_factor(c, st, hb, nullptr, keep_dev);
    launch_backward(c, st, nullptr, nullptr, nullptr, nullptr, nullptr);
    note_factored(c, ns - K.kept, K.kept, K.moved, (int64_t)((now_ms() - t_pick) * 1e6));
    c->inv_valid = false;
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// forward + backward solves with the fronts of the last factorization (the right-hand side from hb)
extern "C" int dpg_chol_resolve(void* h, const double* hb, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(c->sync.p, 0, c->plan.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
    const double* di = c->plan.use_dinv ? c->dinv.p : nullptr;   // inverted by the factorization's dpg_chol_solve
    const double* li = c->inv_valid ? c->linv.p : nullptr;
    launch_forward(c, st, hb, di, nullptr, li);
    launch_backward(c, st, di, nullptr, nullptr, nullptr, li);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// one Gauss-Newton iteration's solve with the path chosen on the device (gate, see gate_off):
// the fused factorization + forward solve, or the forward solve with the last factor, then the
// backward solve.  Only the fused plan without inverted diagonal blocks (dpg_chol_gated_ok).
extern "C" int dpg_chol_gated_ok(void* h) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    return c && c->plan.fused && !(c->plan.use_dinv && c->plan.n_dblocks > 0) ? 1 : 0;
}

extern "C" void dpg_chol_sync_dev(void* h, int32_t** sync, int64_t* n_words) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    *sync = c->sync.p;
    *n_words = (int64_t)(c->plan.sync_bytes / sizeof(int32_t));
}

// prezeroed: the caller's previous launch cleared the status word and the sync counters
extern "C" int dpg_chol_solve_gated(void* h, const double* hb, const int32_t* gate, int prezeroed, double* X,
                                    double* max_out, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!dpg_chol_gated_ok(h)) return DPG_ERR_STATE;
    c->fac_valid = false;   // (a Gauss-Newton loop's refactorizations are not tracked)
    c->has_factor = true;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!prezeroed && (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess ||
                       hipMemsetAsync(c->sync.p, 0, c->plan.sync_bytes, st) != hipSuccess))
        return DPG_ERR_HIP;
    const bool inv = c->plan.n_inv_tasks > 0;
    if (inv) {   // this iteration's solves come after the previous iteration's inverse
        if (!c->aux.s) {
            if (hipStreamCreateWithFlags(&c->aux.s, hipStreamNonBlocking) != hipSuccess ||
                c->ev_fac.ensure(hipEventDisableTiming) || c->ev_inv[0].ensure(hipEventDisableTiming) ||
                c->ev_inv[1].ensure(hipEventDisableTiming) || hipEventRecord(c->ev_inv[0].e, c->aux.s) != hipSuccess ||
                hipEventRecord(c->ev_inv[1].e, c->aux.s) != hipSuccess)
                return DPG_ERR_HIP;
        }
        if (hipStreamWaitEvent(st, c->ev_inv[c->inv_par ^ 1].e, 0) != hipSuccess) return DPG_ERR_HIP;
    }
    launch_factor(c, st, hb, gate, nullptr);
    if (inv) {   // L11^-1 of a refactoring iteration beside its backward solve (which does not use it)
        if (hipEventRecord(c->ev_fac.e, st) != hipSuccess || hipStreamWaitEvent(c->aux.s, c->ev_fac.e, 0) != hipSuccess)
            return DPG_ERR_HIP;
        launch_inv(c, c->aux.s, gate);
        if (hipEventRecord(c->ev_inv[c->inv_par].e, c->aux.s) != hipSuccess) return DPG_ERR_HIP;
        c->inv_par ^= 1;
    }
    launch_forward(c, st, hb, nullptr, gate, c->linv.p);
    launch_backward(c, st, nullptr, gate, X, max_out, c->linv.p);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// a Gauss-Newton graph's solver keeps L11^-1 for its chord steps (the incremental graph refactors
// every update and does not)
extern "C" void dpg_chol_keep_inverse(void* h, int on) {
    if (h) reinterpret_cast<CholDev*>(h)->keep_inv = on != 0;
}

// the gated loop's control kernel rewrites the gate the inverse kernel reads: it must come after
// this iteration's inverse (normally long finished: it ran beside the backward solve and assembly)
extern "C" int dpg_chol_join_aux(void* h, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c || !c->aux.s) return DPG_OK;
    return hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), c->ev_inv[c->inv_par ^ 1].e, 0) == hipSuccess ? DPG_OK
                                                                                                       : DPG_ERR_HIP;
}

extern "C" const int32_t* dpg_chol_pos_dev(void* h) { return reinterpret_cast<CholDev*>(h)->pos; }
extern "C" const double* dpg_chol_x_dev(void* h) { return reinterpret_cast<CholDev*>(h)->xsol.p; }
extern "C" const int32_t* dpg_chol_status_dev(void* h) { return reinterpret_cast<CholDev*>(h)->status.p; }
extern "C" void dpg_chol_stats(void* h, double out[6]) {
    const dpg_chol_sym& S = reinterpret_cast<CholDev*>(h)->sym;
    out[0] = S.ns;
    out[1] = S.n_levels;
    out[2] = S.max_front;
    out[3] = S.flops;
    out[4] = (double)S.front_off[(size_t)S.ns] * 8.0;
    out[5] = (double)S.n;
}

#ifdef DPG_CHOL_TIMING
extern "C" void dpg_chol_tree(void* h, int32_t* parent, int32_t* m3, int32_t* k3) {
    const dpg_chol_sym& S = reinterpret_cast<CholDev*>(h)->sym;
    for (int32_t s = 0; s < S.ns; ++s) {
        parent[s] = S.sn_parent[(size_t)s];
        k3[s] = 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]);
        m3[s] = k3[s] + 3 * (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
    }
}
#endif
