// dpg_gn_api.hip -- the pose-graph half of the extern "C" boundary (include/dpg_slam_c.h): setup,
// poses, the per-iteration step API, the all-reduce forms and the host collective thread, both
// Gauss-Newton loops, run / optimize, marginals and joint marginals.
//
// Entry points replace (reference file:line):
//   dpg_optimize_graph    -> DpgSLAM::optimizeGraph        src/dpg_slam/dpg_slam.cc:316-329
//   dpg_gn_*              -> the same solve, split for the edge-sharded multi-GPU driver

#include <string.h>

#include <chrono>
#include <cmath>

#include "dpg_ctx.h"

static int gn_setup_1(dpg_ctx* c, int64_t V, const dpg_factor* F, int64_t nf, int64_t b, int64_t e,
                      const dpg_gn_params* gp) {
    HIP_TRY(hipSetDevice(c->device));
    // the new graph's host work overlaps what still runs on the stream (a batch's ICP); the
    // stream is drained before the device allocations, and the previous graph released after them
    // (it goes to `ng` in the move and away with it); a failed build leaves the previous graph live
    GnGraph ng;
    int rc = ng.build(V, F, nf, b, e, &c->copts, c->stream);
    if (rc) return fail(rc, "pose-graph setup failed (invalid factor or out of memory)");
    c->gn = std::move(ng);
    c->gn_ready = true;
    c->gn_pairs_valid = false;
    c->gp = or_default(gp, dpg_gn_params_default);
    return DPG_OK;
}

static int gn_set_poses_1(dpg_ctx* c, const double* poses) {
    if (!c->gn_ready) return fail(DPG_ERR_STATE, "graph not set up");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->gn.v.poses, poses, sizeof(double) * 3 * (size_t)c->gn.v.n_nodes, hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->gn.v.have_factor = 0;            // a new linearization point: the next solve refactors
    c->gn.v.last_delta_inf = 1e300;
    c->gn.v.prev_delta_inf = 1e300;
    c->gn.v.last_was_chord = 0;
    c->gn.v.n_factorizations = 0;
    return DPG_OK;
}

// the per-iteration step API: one device, the caller's collective between its calls
#define DPG_STEP_API_1(c)                                                                                        \
    do {                                                                                                         \
        if (!(c) || !(c)->gn_ready) return fail(DPG_ERR_STATE, "graph not set up");                             \
        if (is_multi(c)) return fail(DPG_ERR_STATE, "the step API is per device: a multi-device context runs "   \
                                                    "dpg_gn_run / dpg_optimize_graph / dpg_reoptimize");         \
    } while (0)

// enqueue solve + retract on one device (no multi check: the multi-device host loop uses it per device)
static int solve_retract_async_1(dpg_ctx* c, const double* hb_dev) {
    if (!hb_dev) hb_dev = c->gn.v.hb_own;
    HIP_TRY(hipEventRecord(c->ev[4].e, c->stream));
    int rc = dpg_gn_dev_solve_async(&c->gn.v, hb_dev, &c->gp, c->stream);
    if (rc) return fail(rc, "solve launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipEventRecord(c->ev[5].e, c->stream));
    return DPG_OK;
}

static int fetch_1(dpg_ctx* c, const double* hb_dev, double out[3]) {
    if (!hb_dev) hb_dev = c->gn.v.hb_own;
    int rc = dpg_gn_dev_fetch(&c->gn.v, hb_dev, c->stream, out);
    if (rc) return fail(rc, "fetch failed");
    float s = 0.f;
    if (hipEventElapsedTime(&s, c->ev[4].e, c->ev[5].e) == hipSuccess) c->solve_ms = s;
    return DPG_OK;
}

static int read_error(dpg_ctx* c, double* err) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(err, c->gn.v.hb_own + 9 * c->gn.v.nnzb_upper + 3 * c->gn.v.n_nodes, sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

static int check_conv(const dpg_gn_params* gp, double cur, double nw) {
    if (nw <= 0.0) return 1;
    const double abs_dec = cur - nw;
    const double rel_dec = abs_dec / cur;
    return (gp->relative_error_tol != 0.0 && rel_dec <= gp->relative_error_tol) || (abs_dec <= gp->absolute_error_tol);
}

// The multi-device forms' all-reduce: every local device's hb_part summed into every hb_own --
// ONE ncclAllReduce(sum, fp64) per device on its own stream (grouped: one thread drives them), or
// the virtual devices' rank-order sum.  Out of place, so an iteration that a gate turned into
// no-ops sums the same partial buffers again and leaves hb_own as it was.
static int coll_sum_hb(dpg_ctx* c) {
    const size_t count = (size_t)dpg_gn_dev_hb_size(&c->gn.v);
    if (c->coll == kCollVirtual) {
        const double* parts[kMaxVirtual];
        double* outs[kMaxVirtual];
        for (int k = 0; k < n_dev(c); ++k) {
            parts[k] = dev_ctx(c, k)->gn.v.hb_part;
            outs[k] = dev_ctx(c, k)->gn.v.hb_own;
        }
        const int rc = dpg_launch_vsum(parts, outs, n_dev(c), (int64_t)count, c->stream);   // the shared stream
        return rc ? fail(rc, "virtual all-reduce launch failed") : DPG_OK;
    }
    if (c->coll == kCollHost) {   // the caller's collective, through host memory (blocking)
        c->host_hb.resize(count);
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpyAsync(c->host_hb.data(), c->gn.v.hb_part, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->host_ops.allreduce_sum_f64(c->host_ops.user, c->host_hb.data(), (int64_t)count))
            return fail(DPG_ERR_HIP, "the caller's all-reduce of the packed system failed");
        HIP_TRY(hipMemcpyAsync(c->gn.v.hb_own, c->host_hb.data(), sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return DPG_OK;
    }
    if (ncclGroupStart() != ncclSuccess) return fail(DPG_ERR_HIP, "ncclGroupStart failed");
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        const ncclResult_t r = ncclAllReduce(q->gn.v.hb_part, q->gn.v.hb_own, count, ncclDouble, ncclSum, c->comms[(size_t)k],
                                             q->stream);
        if (r != ncclSuccess) {
            (void)ncclGroupEnd();
            return fail(DPG_ERR_HIP, "ncclAllReduce failed: %s", ncclGetErrorString(r));
        }
    }
    if (ncclGroupEnd() != ncclSuccess) return fail(DPG_ERR_HIP, "ncclGroupEnd failed");
    return DPG_OK;
}

// kCollHost, pipelined GN: the collective thread's loop (see dpg_ctx::HostColl)
static void host_coll_thread(dpg_ctx::HostColl* hp, int device, dpg_coll_ops ops) {
    dpg_ctx::HostColl& h = *hp;
    (void)hipSetDevice(device);
    for (;;) {
        std::pair<uint32_t, hipEvent_t> job;
        {
            std::unique_lock<std::mutex> lk(h.mu);
            h.cv.wait(lk, [&] { return h.stop || !h.jobs.empty(); });
            if (h.jobs.empty()) return;   // stop, nothing left
            job = h.jobs.front();
            h.jobs.pop_front();
        }
        int bad = hipEventSynchronize(job.second) != hipSuccess;
        if (!bad && ops.allreduce_sum_f64(ops.user, h.buf.p, (int64_t)h.count)) bad = 1;
        if (bad) h.failed.store(1);
        std::atomic_thread_fence(std::memory_order_release);   // the sum before the tag
        __atomic_store_n(h.flag.p, job.first, __ATOMIC_RELEASE);
        {
            std::lock_guard<std::mutex> lk(h.mu);
            ++h.done;
        }
        h.cv.notify_all();
    }
}

int dpg_ctx::HostColl::create(const dpg_ctx* c, std::unique_ptr<HostColl>& out) {
    std::unique_ptr<HostColl> h(new HostColl());
    if (h->flag.reserve(2) || h->ev[0].ensure(hipEventDisableTiming) || h->ev[1].ensure(hipEventDisableTiming))
        return fail(DPG_ERR_HIP, "the collective thread's flag words and events could not be created");
    h->flag.p[0] = h->flag.p[1] = 0;
    h->th = std::thread(host_coll_thread, h.get(), c->device, c->host_ops);
    out = std::move(h);
    return DPG_OK;
}

dpg_ctx::HostColl::~HostColl() {
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
}

// queue iteration's all-reduce on the collective thread and make the stream wait for it
static int coll_sum_hb_host_async(dpg_ctx* c) {
    const size_t count = (size_t)dpg_gn_dev_hb_size(&c->gn.v);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (!c->hc && (rc = dpg_ctx::HostColl::create(c, c->hc))) return rc;
    dpg_ctx::HostColl& h = *c->hc;
    // the thread is idle here: every posted job has completed (hc_drain)
    if (h.buf.cap < count && h.buf.reserve(count)) return fail(DPG_ERR_HIP, "hipHostMalloc(collective buffer) failed");
    h.count = count;
    const uint32_t tag = ++h.next_tag;
    hipEvent_t ev = h.ev[tag & 1].e;
    HIP_TRY(hipMemcpyAsync(h.buf.p, c->gn.v.hb_part, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev, c->stream));
    {
        std::lock_guard<std::mutex> lk(h.mu);
        h.jobs.emplace_back(tag, ev);
        ++h.posted;
    }
    h.cv.notify_all();
    rc = dpg_launch_host_wait(h.flag.p, tag, h.flag.p + 1, c->stream);
    if (rc) return fail(rc, "host-collective wait launch failed");
    HIP_TRY(hipMemcpyAsync(c->gn.v.hb_own, h.buf.p, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    return DPG_OK;
}

// every all-reduce posted to the collective thread has completed (its stream work may still run)
static void hc_drain(dpg_ctx* c) {
    if (!c->hc) return;
    std::unique_lock<std::mutex> lk(c->hc->mu);
    c->hc->cv.wait(lk, [&] { return c->hc->done == c->hc->posted; });
}

static int ensure_pipe(dpg_ctx* q) {
    if (q->pipe_slot.p) return DPG_OK;   // (made last)
    HIP_TRY(hipSetDevice(q->device));
    if (q->pipe_ctl.reserve(1) || q->pipe_slot.reserve(3))   // + [2]: the initial error
        return fail(DPG_ERR_HIP, "GN pipeline: allocating the control block and report slots failed");
    memset(q->pipe_slot.p, 0, 3 * sizeof(dpg_gn_slot));
    return DPG_OK;
}

// Wait for the report tagged `tag` in a host-mapped slot (the device stores the tag last, after a
// system-scope fence).  Spins, then yields; every ~2 ms checks the stream: a stream that has
// drained (or failed) without posting the tag is an error, not a hang.
static int wait_slot(dpg_ctx* q, const dpg_gn_slot* slot, uint64_t tag) {
    const volatile uint64_t* t = &slot->tag;
    auto t0 = std::chrono::steady_clock::now(), last = t0;
    for (unsigned n = 0;; ++n) {
        if (*t == tag) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return DPG_OK;
        }
        if (n < 4096) {
            __builtin_ia32_pause();
            continue;
        }
        std::this_thread::yield();
        const auto now = std::chrono::steady_clock::now();
        if (now - last > std::chrono::milliseconds(2)) {
            last = now;
            const hipError_t e = hipStreamQuery(q->stream);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(DPG_ERR_HIP, "GN pipeline: %s", hipGetErrorString(e));
            if (e == hipSuccess && *t != tag) return fail(DPG_ERR_STATE, "GN pipeline: the stream drained without the report");
            if (now - t0 > std::chrono::seconds(60)) return fail(DPG_ERR_HIP, "GN pipeline: no report after 60 s");
        }
    }
}

// The Gauss-Newton iterations with the decisions on the device (dpg_gn_pipe.h): iteration k + 1 is
// queued before iteration k's report is read, so the GPU never waits for the host.  Multi-device
// forms: every device solves the identical all-reduced system and decides for itself (its own
// control block: the chord rule's bookkeeping stays per device); their reports must agree bit for
// bit, which the loop checks every iteration.
static int gn_loop_pipe_body(dpg_ctx* c, const dpg_gn_params& P, dpg_gn_stats& S, double& nw, double& dinf, int& it);
static int gn_loop_pipe(dpg_ctx* c, const dpg_gn_params& P, dpg_gn_stats& S, double& nw, double& dinf, int& it) {
    int rc = gn_loop_pipe_body(c, P, S, nw, dinf, it);
    if (c->coll == kCollHost && c->hc) {   // nothing of this loop left on the collective thread
        hc_drain(c);
        if (!rc && c->hc->failed.exchange(0)) rc = fail(DPG_ERR_HIP, "the caller's all-reduce of the packed system failed");
        if (!rc && __atomic_load_n(c->hc->flag.p + 1, __ATOMIC_ACQUIRE))
            rc = fail(DPG_ERR_HIP, "GN pipeline: no all-reduce from the collective thread in 120 s");
    }
    return rc;
}
static int gn_loop_pipe_body(dpg_ctx* c, const dpg_gn_params& P, dpg_gn_stats& S, double& nw, double& dinf, int& it) {
    const int L = n_dev(c);
    const int part = is_multi(c) ? 1 : 0;
    int rc;
    for (int k = 0; k < L; ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        if ((rc = ensure_pipe(q))) return rc;
        ++q->pipe_loop;
        const double* cur_dev = q->gn.v.hb_own + 9 * q->gn.v.nnzb_upper + 3 * q->gn.v.n_nodes;   // the assembled error
        if ((rc = dpg_gn_pipe_init(&q->gn.v, &P, q->pipe_ctl.p, cur_dev, q->pipe_slot.p + 2, q->pipe_loop, q->stream)))
            return fail(rc, "GN pipeline launch failed");
    }
    auto issue = [&](int i) -> int {   // iteration i (1-based) reports into slot i & 1
        int r;
        for (int k = 0; k < L; ++k) {
            dpg_ctx* q = dev_ctx(c, k);
            HIP_TRY(hipSetDevice(q->device));
            if ((r = dpg_gn_pipe_issue_solve(&q->gn.v, q->pipe_ctl.p, part, q->stream)))
                return fail(r, "GN pipeline launch failed: %s", hipGetErrorString(hipGetLastError()));
        }
        if (part && (r = (c->coll == kCollHost ? coll_sum_hb_host_async(c) : coll_sum_hb(c)))) return r;
        for (int k = 0; k < L; ++k) {
            dpg_ctx* q = dev_ctx(c, k);
            HIP_TRY(hipSetDevice(q->device));
            if ((r = dpg_gn_pipe_issue_ctl(&q->gn.v, &P, q->pipe_ctl.p, q->pipe_slot.p + (i & 1), part, q->stream)))
                return fail(r, "GN pipeline launch failed: %s", hipGetErrorString(hipGetLastError()));
        }
        return DPG_OK;
    };
    if ((rc = issue(1))) return rc;
    int issued = 1;
    std::vector<int> nfact((size_t)L, 0), reuse_last((size_t)L, 0);
    for (int k = 0; k < L; ++k) reuse_last[(size_t)k] = dev_ctx(c, k)->gn.v.last_was_chord;
    for (int i = 1;; ++i) {
        if (issued < P.max_iterations) {
            if ((rc = issue(i + 1))) return rc;
            ++issued;
        }
        dpg_gn_slot o0{};
        for (int k = 0; k < L; ++k) {
            dpg_ctx* q = dev_ctx(c, k);
            HIP_TRY(hipSetDevice(q->device));
            if (i == 1) {   // the initial error, as the device read it (pipe_init_kernel)
                if ((rc = wait_slot(q, q->pipe_slot.p + 2, (uint64_t)q->pipe_loop << 32))) return rc;
                const double e0 = static_cast<const volatile dpg_gn_slot*>(q->pipe_slot.p + 2)->error;
                if (e0 <= 0.0) {   // nothing to do: no iteration runs (pipe_init_kernel's test, NaN runs)
                    for (int j = 0; j < L; ++j) (void)hipStreamSynchronize(dev_ctx(c, j)->stream);
                    S.initial_error = e0;
                    nw = e0;
                    dinf = 0.0;
                    it = 0;
                    HIP_TRY(hipSetDevice(c->device));
                    return DPG_OK;
                }
            }
            if ((rc = wait_slot(q, q->pipe_slot.p + (i & 1), ((uint64_t)q->pipe_loop << 32) | (uint32_t)i))) return rc;
            dpg_gn_slot o;   // host-mapped, written by the device: read through volatile
            {
                const volatile dpg_gn_slot* v = q->pipe_slot.p + (i & 1);
                o.dinf = v->dinf;
                o.error = v->error;
                o.status = v->status;
                o.reuse = v->reuse;
                o.active = v->active;
                o.final_ = v->final_;
                o.it = v->it;
            }
            if (i == 1 && k == 0) S.initial_error = static_cast<const volatile dpg_gn_slot*>(q->pipe_slot.p + 2)->error;
            if (!o.active || o.it != i) return fail(DPG_ERR_STATE, "GN pipeline out of step (device %d, iteration %d)", k, i);
            if (k == 0) {
                o0 = o;
            } else if (memcmp(&o.dinf, &o0.dinf, sizeof(double)) || memcmp(&o.error, &o0.error, sizeof(double)) ||
                       o.status != o0.status || o.reuse != o0.reuse || o.final_ != o0.final_) {
                for (int j = 0; j < L; ++j) (void)hipStreamSynchronize(dev_ctx(c, j)->stream);
                return fail(DPG_ERR_INTERNAL, "devices diverged at GN iteration %d (device %d: |d| %.17g error %.17g, "
                            "device 0: %.17g %.17g)", i, k, o.dinf, o.error, o0.dinf, o0.error);
            }
            if (!o.reuse) ++nfact[(size_t)k];
            q->gn.v.prev_delta_inf = q->gn.v.last_delta_inf;
            q->gn.v.last_delta_inf = o.dinf;
            reuse_last[(size_t)k] = o.reuse;
        }
        if (c->hc && c->hc->failed.load()) {   // the caller's collective failed: the report is not a sum
            for (int j = 0; j < L; ++j) (void)hipStreamSynchronize(dev_ctx(c, j)->stream);
            return fail(DPG_ERR_HIP, "the caller's all-reduce of the packed system failed (GN iteration %d)", i);
        }
        if (o0.status != 0.0) {
            for (int j = 0; j < L; ++j) (void)hipStreamSynchronize(dev_ctx(c, j)->stream);
            if (o0.status == (double)DPG_GN_STATUS_DIVERGED)
                return fail(DPG_ERR_INTERNAL, "ranks diverged at GN iteration %d (different max |delta| in the vote words)", i);
            return fail(DPG_ERR_NUMERIC, "Cholesky failed (status %d)", (int)o0.status);
        }
        it = i;
        dinf = o0.dinf;
        nw = o0.error;
        if (o0.final_) break;
    }
    // the host bookkeeping the step API continues from (as after the host loop)
    for (int k = 0; k < L; ++k) {
        dpg_gn_dev* g = &dev_ctx(c, k)->gn.v;
        g->last_was_chord = reuse_last[(size_t)k];
        g->have_factor = 1;
        g->n_factorizations += nfact[(size_t)k];
        g->last_used_chol = 1;
    }
    S.pcg_iterations = 0;
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

static bool pipe_ok(dpg_ctx* c, const dpg_gn_params& P) {
    if (P.linear_solver != DPG_SOLVER_CHOLESKY) return false;
    for (int k = 0; k < n_dev(c); ++k) {
        const dpg_gn_dev& g = dev_ctx(c, k)->gn.v;
        if (!g.chol || !dpg_chol_gated_ok(g.chol)) return false;
    }
    return true;
}

// The Gauss-Newton loop on a set-up graph whose poses are set.  One device: assemble, then the
// pipelined iterations (or, for the PCG solver / a factorization that cannot run gated, the
// host-decided loop: solve + retract + re-linearize enqueued back to back, ONE read per iteration).
// Multi-device forms: the same loops with every device's share assembled into its hb_part and ONE
// all-reduce into hb_own between the assembly and the decision; every device solves the identical
// system, so the poses stay bitwise equal on all of them without a broadcast.
int gn_loop(dpg_ctx* c, const dpg_gn_params& P, double* poses, double t0, double t1, dpg_gn_stats* st) {
    dpg_gn_stats S;
    memset(&S, 0, sizeof(S));
    const int L = n_dev(c);
    const bool multi = is_multi(c);
    int rc;
    for (int k = 0; k < L; ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        HIP_TRY(hipSetDevice(q->device));
        if (multi) rc = dpg_gn_dev_assemble_part(&q->gn.v, nullptr, q->stream);
        else rc = dpg_gn_dev_assemble(&q->gn.v, q->gn.v.hb_own, q->stream);
        if (rc) return fail(rc, "assembly launch failed");
    }
    if (multi && (rc = coll_sum_hb(c))) return rc;
    double cur = 0.0, nw = 0.0, dinf = 0.0;
    int it = 0;
    const bool pipe = pipe_ok(c, P) && P.max_iterations > 0;
    if (!pipe) {   // (the pipelined loop takes the initial error on the device: no round trip)
        if ((rc = read_error(c, &S.initial_error))) return rc;
        cur = nw = S.initial_error;
    }
    if (pipe) {
        if ((rc = gn_loop_pipe(c, P, S, nw, dinf, it))) return rc;
    } else if (!(cur <= 0.0) && P.max_iterations > 0) {
        for (;;) {
            for (int k = 0; k < L; ++k) {
                dpg_ctx* q = dev_ctx(c, k);
                HIP_TRY(hipSetDevice(q->device));
                if ((rc = solve_retract_async_1(q, nullptr))) return rc;
                if (multi) rc = dpg_gn_dev_assemble_part(&q->gn.v, nullptr, q->stream);
                else rc = dpg_gn_dev_assemble(&q->gn.v, q->gn.v.hb_own, q->stream);
                if (rc) return fail(rc, "assembly launch failed");
            }
            if (multi && (rc = coll_sum_hb(c))) return rc;
            // every device reads its own scalars: its chord rule's bookkeeping (last / previous
            // max|delta|) moves with its own solves, and the devices must agree
            double sc0[3] = {0, 0, 0};
            for (int k = 0; k < L; ++k) {
                dpg_ctx* q = dev_ctx(c, k);
                double sc[3];
                HIP_TRY(hipSetDevice(q->device));
                if ((rc = fetch_1(q, nullptr, sc))) return rc;
                if (k == 0) memcpy(sc0, sc, sizeof(sc));
                else if (memcmp(sc, sc0, sizeof(sc)))
                    return fail(DPG_ERR_INTERNAL, "devices diverged at GN iteration %d (device %d)", it + 1, k);
            }
            // world > 1: decide from the all-reduced vote words (every rank's max |delta| and
            // status of this iteration, dpg_gn.hip chi2_kernel), never from the local scalars
            // alone -- ranks that disagreed would issue different numbers of all-reduces and hang
            if (multi && c->gn.v.n_vote > 0) {
                const int W = c->gn.v.world;
                std::vector<double> vw((size_t)(2 * W));
                HIP_TRY(hipSetDevice(c->device));
                HIP_TRY(hipMemcpyAsync(vw.data(), c->gn.v.hb_own + dpg_gn_dev_vote_offset(&c->gn.v), sizeof(double) * vw.size(),
                                       hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                for (int r = 0; r < W; ++r) {
                    if (memcmp(&vw[(size_t)r], &vw[0], sizeof(double)))
                        return fail(DPG_ERR_INTERNAL, "ranks diverged at GN iteration %d (rank %d: |d| %.17g, rank 0: %.17g)",
                                    it + 1, r, vw[(size_t)r], vw[0]);
                    sc0[2] = std::max(sc0[2], vw[(size_t)(W + r)]);
                }
                sc0[0] = vw[0];
            }
            if (sc0[2] != 0.0) return fail(DPG_ERR_NUMERIC, "Cholesky failed (status %d)", (int)sc0[2]);
            S.pcg_iterations += c->gn.v.last_pcg_iters;
            ++it;
            dinf = sc0[0];
            nw = sc0[1];
            if (it >= P.max_iterations) break;
            if (P.use_error_criteria) {
                if (check_conv(&P, cur, nw) || !std::isfinite(cur)) break;
            } else if (dinf < P.delta_tol) {
                break;
            }
            cur = nw;
        }
    }
    if (multi && (rc = dpg_ctx_synchronize(c))) return rc;
    if (poses && (rc = dpg_gn_get_poses(c, poses))) return rc;
    if (!poses) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const double t2 = now_ms();
    S.iterations = it;
    S.final_error = nw;
    S.last_delta_inf = dinf;
    S.ms_total = t2 - t0;
    S.ms_per_iteration = it ? (t2 - t1) / it : 0.0;
    if (st) *st = S;
    return DPG_OK;
}

// ---- marginal covariances (gtsam::Marginals, dpg_slam_main.cc:272-279) ----
// The graph of the last setup is linearized at its current poses and factored (a chord step may
// have left the factor of an earlier iterate; Marginals linearizes at the values it is given),
// then the selected inverse of that factor gives the blocks (dpg_chol.hip).  The loop's state is
// left alone: poses, step sizes, the factorization count and whether it holds a factor at all
// (after dpg_gn_set_poses it does not, and its first solve factors as it would have anyway; a
// factor it did hold is replaced by the one at the current poses).
static int gn_marginals_state(dpg_ctx* c, const char* fn) {
    if (!c || !c->gn_ready) return fail(DPG_ERR_STATE, "%s: graph not set up", fn);
    if (is_multi(c)) return fail(DPG_ERR_STATE, "%s: marginals are single-device (this context has several ranks)", fn);
    if (c->gp.linear_solver != DPG_SOLVER_CHOLESKY || !c->gn.v.chol)
        return fail(DPG_ERR_STATE, "%s: the graph has no Cholesky factorization (linear_solver)", fn);
    return DPG_OK;
}

// the front half of both marginals paths, after their checks: linearize at the current poses and
// factor (timed: ev[3] .. ev[4] the assembly, ev[4] .. ev[5] the factorization)
static int gn_factor_at_current_poses(dpg_ctx* c, const char* fn, bool timed) {
    HIP_TRY(hipSetDevice(c->device));
    dpg_gn_dev* g = &c->gn.v;
    int rc;
    if (timed) HIP_TRY(hipEventRecord(c->ev[3].e, c->stream));
    if ((rc = dpg_gn_dev_assemble(g, g->hb_own, c->stream))) return fail(rc, "%s: assembly launch failed", fn);
    if (timed) HIP_TRY(hipEventRecord(c->ev[4].e, c->stream));
    if ((rc = dpg_chol_solve(g->chol, g->hb_own, c->stream))) return fail(rc, "%s: factorization launch failed", fn);
    if (timed) HIP_TRY(hipEventRecord(c->ev[5].e, c->stream));
    return DPG_OK;
}

static int gn_marginals_blocks(dpg_ctx* c, const char* fn, const int32_t* nodes, int64_t n, const int32_t* pairs,
                               int64_t n_pairs, double* out, double* ms) {
    int rc = gn_marginals_state(c, fn);
    if (rc) return rc;
    if (!out || n < 0 || n_pairs < 0) return fail(DPG_ERR_ARG, "%s: bad arguments", fn);
    if (dpg_chol_selinv_check(c->gn.v.chol, nodes, n, pairs, n_pairs))
        return fail(DPG_ERR_ARG, "%s: a node is out of range or a pair's block is outside the factor's pattern", fn);
    if ((rc = gn_factor_at_current_poses(c, fn, ms != nullptr))) return rc;
    rc = dpg_chol_marginals(c->gn.v.chol, nodes, n, pairs, n_pairs, out, c->stream);
    if (rc == DPG_ERR_NUMERIC) return fail(rc, "%s: H is not positive definite", fn);
    if (rc) return fail(rc, "%s: selected inversion failed", fn);
    if (ms) {
        float a = 0.f, f = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, c->ev[3].e, c->ev[4].e));
        HIP_TRY(hipEventElapsedTime(&f, c->ev[4].e, c->ev[5].e));
        ms[0] = a;
        ms[1] = f;
    }
    return DPG_OK;
}

// the pairs must share a factor (H's own pattern): blocks that only fill or a relaxed supernode put
// into L's pattern are not part of the interface
static int gn_pairs_share_factor(dpg_ctx* c, const int32_t* pairs, int64_t n) {
    const dpg_gn_dev& g = c->gn.v;
    if (!c->gn_pairs_valid) {
        HIP_TRY(hipSetDevice(c->device));
        std::vector<dpg_factor> F((size_t)g.n_factors);
        if (g.n_factors > 0) {
            HIP_TRY(hipMemcpyAsync(F.data(), g.factors, sizeof(dpg_factor) * F.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        c->gn_pairs.clear();
        for (const dpg_factor& f : F)
            if (f.kind == DPG_FACTOR_BETWEEN && f.i != f.j)
                c->gn_pairs.push_back((uint64_t)(uint32_t)std::min(f.i, f.j) << 32 | (uint32_t)std::max(f.i, f.j));
        std::sort(c->gn_pairs.begin(), c->gn_pairs.end());
        c->gn_pairs.erase(std::unique(c->gn_pairs.begin(), c->gn_pairs.end()), c->gn_pairs.end());
        c->gn_pairs_valid = true;
    }
    for (int64_t q = 0; q < n; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || j < 0 || i >= g.n_nodes || j >= g.n_nodes)
            return fail(DPG_ERR_ARG, "dpg_gn_marginal_pairs: pair %lld has a node out of range", (long long)q);
        if (i != j && !std::binary_search(c->gn_pairs.begin(), c->gn_pairs.end(),
                                          (uint64_t)(uint32_t)std::min(i, j) << 32 | (uint32_t)std::max(i, j)))
            return fail(DPG_ERR_ARG, "dpg_gn_marginal_pairs: nodes %d and %d share no factor", i, j);
    }
    return DPG_OK;
}

// ---- joint marginals and relative-pose covariances of any node pair (Marginals::jointMarginalCovariance) ----
// The same linearization and factorization as above, then the blocks from root paths of the factor
// (dpg_chol_joint): no pattern restriction.  The relative-pose Jacobian is 3x3 arithmetic per pair
// on the host (dpg_relative_covariance), at the poses the factor was linearized at.
static int gn_joint_blocks(dpg_ctx* c, const char* fn, int by_nodes, const int32_t* idx, int64_t n, double* out, float* ms) {
    int rc = gn_marginals_state(c, fn);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!idx || !out))) return fail(DPG_ERR_ARG, "%s: bad arguments", fn);
    for (int64_t q = 0, e = by_nodes ? n : 2 * n; q < e; ++q)
        if (idx[q] < 0 || idx[q] >= c->gn.v.n_nodes) return fail(DPG_ERR_ARG, "%s: node %d is out of range", fn, idx[q]);
    if (n == 0) return DPG_OK;
    if ((rc = gn_factor_at_current_poses(c, fn, false))) return rc;
    rc = dpg_chol_joint(c->gn.v.chol, by_nodes, idx, n, out, c->stream, ms);
    if (rc == DPG_ERR_NUMERIC) return fail(rc, "%s: H is not positive definite", fn);
    if (rc) return fail(rc, "%s: the path solve failed", fn);
    return DPG_OK;
}

extern "C" {

// Multi-device forms: every local device holds the whole factor list (the sparsity pattern is
// global) and linearizes the factors f with f mod world == its rank; dpg_gn_take_icp_measurements
// then hands each ICP slot to the device that aligned the edge.
int dpg_gn_setup(dpg_ctx* c, int64_t V, const dpg_factor* F, int64_t nf, int64_t b, int64_t e,
                 const dpg_gn_params* gp) {
    if (!c || !F || V <= 0 || nf < 0) return fail(DPG_ERR_ARG, "dpg_gn_setup: bad arguments");
    if (!is_multi(c)) return gn_setup_1(c, V, F, nf, b, e, gp);
    if (b != 0 || e != nf) return fail(DPG_ERR_ARG, "dpg_gn_setup: a multi-device context shards the factors itself (0, n_factors)");
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        int rc = gn_setup_1(q, V, F, nf, 0, nf, gp);
        if (!rc && (rc = dpg_gn_dev_set_ownership(&q->gn, c->world, q->rank, q->stream)))
            rc = fail(rc, "pose-graph ownership setup failed");
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

int dpg_gn_take_icp_measurements(dpg_ctx* c, int64_t first, int64_t count, int64_t n_always,
                                 const dpg_icp_params* p) {
    if (!c || !c->gn_ready || !p) return fail(DPG_ERR_STATE, "graph not set up");
    const double ix = 1.0 / (double)p->laser_x_variance, iy = 1.0 / (double)p->laser_y_variance,
                 ith = 1.0 / (double)p->laser_theta_variance;
    if (!is_multi(c)) {
        if (count > c->n_edges) return fail(DPG_ERR_ARG, "only %lld ICP results available", (long long)c->n_edges);
        int rc = dpg_gn_dev_icp_to_factors(&c->gn.v, c->res.p, first, count, n_always, ix, iy, ith, c->stream);
        return rc ? fail(rc, "dpg_gn_take_icp_measurements failed") : DPG_OK;
    }
    // every slot of the batch: the aligning device's result, on that device only
    if (count != (int64_t)c->batch.size())
        return fail(DPG_ERR_ARG, "a multi-device context takes the whole batch (%lld results), not %lld",
                    (long long)c->batch.size(), (long long)count);
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        HIP_TRY(hipSetDevice(q->device));
        if (!q->gn_ready || !q->gn.v.mine) return fail(DPG_ERR_STATE, "graph not set up on device %d", k);
        const int64_t nl = (int64_t)c->shard[(size_t)k].size();
        const int rc = dpg_gn_dev_icp_to_factors_scatter(&q->gn.v, q->res.p, q->shard_idx.p, nl, first, count, n_always,
                                                         ix, iy, ith, q->stream);
        if (rc) return fail(rc, "dpg_gn_take_icp_measurements failed");
    }
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

int64_t dpg_gn_hb_size(dpg_ctx* c) { return (c && c->gn_ready) ? dpg_gn_dev_hb_size(&c->gn.v) : -1; }

int dpg_gn_setup_profile(dpg_ctx* c, double out[5]) {
    if (!c || !c->gn_ready || !out) return fail(DPG_ERR_STATE, "graph not set up");
    for (int k = 0; k < 5; ++k) out[k] = c->gn.v.setup_ms[k];
    return DPG_OK;
}

int dpg_gn_set_poses(dpg_ctx* c, const double* poses) {
    if (!c || !c->gn_ready || !poses) return fail(DPG_ERR_STATE, "graph not set up");
    for (int k = 0; k < n_dev(c); ++k) {
        const int rc = gn_set_poses_1(dev_ctx(c, k), poses);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

int dpg_gn_get_poses(dpg_ctx* c, double* poses) {
    if (!c || !c->gn_ready || !poses) return fail(DPG_ERR_STATE, "graph not set up");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(poses, c->gn.v.poses, sizeof(double) * 3 * (size_t)c->gn.v.n_nodes, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

int dpg_gn_assemble(dpg_ctx* c, double* hb_dev) {
    DPG_STEP_API_1(c);
    if (!hb_dev) hb_dev = c->gn.v.hb_own;
    HIP_TRY(hipEventRecord(c->ev[3].e, c->stream));
    int rc = dpg_gn_dev_assemble(&c->gn.v, hb_dev, c->stream);
    if (rc) return fail(rc, "assembly launch failed");
    HIP_TRY(hipEventRecord(c->ev[4].e, c->stream));
    return DPG_OK;
}

int dpg_gn_solve_retract(dpg_ctx* c, const double* hb_dev, double* delta_inf, double* error, int32_t* pcg_iters) {
    DPG_STEP_API_1(c);
    if (!hb_dev) hb_dev = c->gn.v.hb_own;
    int rc = dpg_gn_dev_solve(&c->gn.v, hb_dev, &c->gp, c->stream, delta_inf, error, pcg_iters);
    if (rc) return fail(rc, "PCG solve failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipEventRecord(c->ev[5].e, c->stream));
    float a = 0.f, s = 0.f;
    if (hipEventSynchronize(c->ev[5].e) == hipSuccess) {
        (void)hipEventElapsedTime(&a, c->ev[3].e, c->ev[4].e);
        (void)hipEventElapsedTime(&s, c->ev[4].e, c->ev[5].e);
    }
    c->asm_ms = a;
    c->solve_ms = s;
    return DPG_OK;
}

int dpg_gn_solve_retract_async(dpg_ctx* c, const double* hb_dev) {
    DPG_STEP_API_1(c);
    return solve_retract_async_1(c, hb_dev);
}

int32_t dpg_gn_factorizations(dpg_ctx* c) { return (c && c->gn_ready) ? c->gn.v.n_factorizations : -1; }

int dpg_gn_fetch(dpg_ctx* c, const double* hb_dev, double out[3]) {
    DPG_STEP_API_1(c);
    if (!out) return fail(DPG_ERR_ARG, "dpg_gn_fetch: out is NULL");
    return fetch_1(c, hb_dev, out);
}

float dpg_gn_last_assemble_ms(dpg_ctx* c) { return c ? c->asm_ms : -1.f; }
float dpg_gn_last_solve_ms(dpg_ctx* c) { return c ? c->solve_ms : -1.f; }

// The GN loop on the graph staged by dpg_gn_setup (+ dpg_gn_take_icp_measurements) from the poses
// of dpg_gn_set_poses, with the setup's parameters: what a host loop over the step API does,
// natively (no interpreter between the launches; multi-device forms: sharded, one all-reduce per
// iteration)
int dpg_gn_run(dpg_ctx* c, double* poses_out, dpg_gn_stats* st) {
    if (!c || !c->gn_ready) return fail(DPG_ERR_STATE, "dpg_gn_run: graph not set up");
    HIP_TRY(hipSetDevice(c->device));
    const double t0 = now_ms();
    return gn_loop(c, c->gp, poses_out, t0, t0, st);
}

int dpg_optimize_graph(dpg_ctx* c, double* poses, int64_t V, const dpg_factor* F, int64_t nf, const dpg_gn_params* gp,
                       dpg_gn_stats* st) {
    const double t0 = now_ms();
    const dpg_gn_params P = or_default(gp, dpg_gn_params_default);
    if (!c || !F || !poses || V <= 0 || nf < 0) return fail(DPG_ERR_ARG, "dpg_optimize_graph: bad arguments");
    int rc = dpg_gn_setup(c, V, F, nf, 0, nf, &P);
    if (rc) return rc;
    if ((rc = dpg_gn_set_poses(c, poses))) return rc;
    return gn_loop(c, P, poses, t0, now_ms(), st);
}

int dpg_gn_marginals(dpg_ctx* c, const int32_t* nodes, int64_t n, double* cov_out) {
    if (c && c->gn_ready && !nodes && n != c->gn.v.n_nodes)
        return fail(DPG_ERR_ARG, "dpg_gn_marginals: nodes == NULL asks for every node (n = %lld)", (long long)c->gn.v.n_nodes);
    return gn_marginals_blocks(c, "dpg_gn_marginals", nodes, n, nullptr, 0, cov_out, nullptr);
}

int dpg_gn_marginal_pairs(dpg_ctx* c, const int32_t* pairs, int64_t n, double* cov_out) {
    if (n > 0 && !pairs) return fail(DPG_ERR_ARG, "dpg_gn_marginal_pairs: pairs is NULL");
    int rc = gn_marginals_state(c, "dpg_gn_marginal_pairs");
    if (rc) return rc;
    if (n < 0 || !cov_out) return fail(DPG_ERR_ARG, "dpg_gn_marginal_pairs: bad arguments");
    if ((rc = gn_pairs_share_factor(c, pairs, n))) return rc;
    return gn_marginals_blocks(c, "dpg_gn_marginal_pairs", nullptr, 0, pairs, n, cov_out, nullptr);
}

int dpg_gn_cross_covariances(dpg_ctx* c, const int32_t* pairs, int64_t n, double* cov_out) {
    return gn_joint_blocks(c, "dpg_gn_cross_covariances", 0, pairs, n, cov_out, nullptr);
}

int dpg_gn_joint_marginal(dpg_ctx* c, const int32_t* nodes, int64_t n, double* cov_out) {
    return gn_joint_blocks(c, "dpg_gn_joint_marginal", 1, nodes, n, cov_out, nullptr);
}

int dpg_gn_relative_covariances(dpg_ctx* c, const int32_t* pairs, int64_t n, double* cov_out) {
    const char* fn = "dpg_gn_relative_covariances";
    int rc = gn_marginals_state(c, fn);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!pairs || !cov_out))) return fail(DPG_ERR_ARG, "%s: bad arguments", fn);
    if (n == 0) return DPG_OK;
    for (int64_t q = 0; q < 2 * n; ++q)
        if (pairs[q] < 0 || pairs[q] >= c->gn.v.n_nodes) return fail(DPG_ERR_ARG, "%s: node %d is out of range", fn, pairs[q]);
    std::vector<int32_t> tri((size_t)(6 * n));
    dpg_relative_triples(pairs, n, tri.data());
    std::vector<double> blocks((size_t)(27 * n)), X((size_t)(3 * c->gn.v.n_nodes));
    if ((rc = gn_joint_blocks(c, fn, 0, tri.data(), 3 * n, blocks.data(), nullptr))) return rc;
    if ((rc = dpg_gn_get_poses(c, X.data()))) return rc;
    dpg_relative_from_blocks(pairs, n, X.data(), blocks.data(), cov_out);
    return DPG_OK;
}

/* Diagnostic (tools/joint_probe.py): one dpg_gn_cross_covariances with its two kernels timed by HIP
 * events.  out = {path solve ms, dot ms, the longest root path in fronts, in pivot scalars}. */
int dpg_gn_joint_profile(dpg_ctx* c, const int32_t* pairs, int64_t n, double* out, int64_t cap) {
    if (!out || cap < 4 || n <= 0) return fail(DPG_ERR_ARG, "dpg_gn_joint_profile: bad arguments");
    std::vector<double> cov((size_t)(9 * n));
    float ms[2] = {0.f, 0.f};
    const int rc = gn_joint_blocks(c, "dpg_gn_joint_profile", 0, pairs, n, cov.data(), ms);
    if (rc) return rc;
    int64_t st[2];
    dpg_chol_path_stats(c->gn.v.chol, st);
    out[0] = ms[0];
    out[1] = ms[1];
    out[2] = (double)st[0];
    out[3] = (double)st[1];
    return DPG_OK;
}

int dpg_marginal_covariances(dpg_ctx* c, const double* poses, int64_t V, const dpg_factor* F, int64_t nf,
                             const int32_t* nodes, int64_t n, double* cov_out) {
    if (!c || !F || !poses || !cov_out || V <= 0 || nf < 0 || n < 0 || (!nodes && n != V))
        return fail(DPG_ERR_ARG, "dpg_marginal_covariances: bad arguments");
    if (is_multi(c)) return fail(DPG_ERR_STATE, "dpg_marginal_covariances: marginals are single-device");
    for (int64_t q = 0; nodes && q < n; ++q)
        if (nodes[q] < 0 || nodes[q] >= V) return fail(DPG_ERR_ARG, "dpg_marginal_covariances: node %lld out of range", (long long)q);
    int rc = dpg_gn_setup(c, V, F, nf, 0, nf, nullptr);
    if (rc) return rc;
    if ((rc = dpg_gn_set_poses(c, poses))) return rc;
    return dpg_gn_marginals(c, nodes, n, cov_out);
}

/* Diagnostic (tools/marginals_probe.py): dpg_gn_marginals of every node with its parts timed by HIP
 * events.  out = {assembly ms, factorization + solve ms, levels, Sigma + work buffer bytes, then the
 * selected inversion's launches, roots' level first}; returns the number of values written. */
int64_t dpg_gn_marginals_profile(dpg_ctx* c, double* out, int64_t cap) {
    int rc = gn_marginals_state(c, "dpg_gn_marginals_profile");
    if (rc) return rc;
    if (!out || cap < 4) return fail(DPG_ERR_ARG, "dpg_gn_marginals_profile: bad arguments");
    std::vector<double> cov((size_t)(9 * c->gn.v.n_nodes));
    double ms[2];
    if ((rc = gn_marginals_blocks(c, "dpg_gn_marginals_profile", nullptr, c->gn.v.n_nodes, nullptr, 0, cov.data(), ms)))
        return rc;
    double st[6];
    dpg_chol_stats(c->gn.v.chol, st);
    const int nl = (int)st[1];
    std::vector<float> lv((size_t)nl, 0.f);
    if ((rc = dpg_chol_selinv_timed(c->gn.v.chol, c->stream, lv.data(), nl))) return fail(rc, "selected inversion failed");
    out[0] = ms[0];
    out[1] = ms[1];
    out[2] = nl;
    out[3] = (double)dpg_chol_selinv_bytes(c->gn.v.chol);
    int64_t k = 4;
    for (int q = 0; q < nl && k < cap; ++q) out[k++] = lv[(size_t)q];
    return k;
}

}  // extern "C"
