// dpg_ctx.hip -- the context half of the extern "C" boundary (include/dpg_slam_c.h): error text,
// version, the five context forms, options, stream, children, and the host-only shard planner.
// Host memory in, host memory out; device work is asynchronous on the context stream except
// where a host value must be returned.  No fallback: without a usable GPU dpg_ctx_create returns
// NULL and every call that needs one fails with DPG_ERR_HIP.

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "dpg_ctx.h"

namespace {
thread_local std::string g_err;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

dpg_ctx* g_default_ctx = nullptr;

// a context form that fails: the message is set, there is no context
static dpg_ctx* no_ctx(int) { return nullptr; }

extern "C" {

const char* dpg_last_error(void) { return g_err.c_str(); }

// internal (dpg_internal.h): error reporting for the translation units without dpg_ctx.h
int dpg_set_error(int code, const char* msg) { return fail(code, "%s", msg); }
const char* dpg_version(void) { return "dpg-mi355x 0.1 (gfx950)"; }

// The batch over the ranks (host only).  cost != NULL: longest-processing-time -- edges by cost,
// longest first (stable: lower index first among equals), each to the least-loaded rank (lower rank
// among equals), dispatched on its rank in that order, so the alignments that bound a launch start
// first.  cost == NULL: edge e on rank e mod world in the caller's order (the caller's lists come
// grouped -- successive pairs, then loop closures nearest first -- so every rank gets the same mix).
int dpg_shard_plan(const float* cost, int64_t ne, int32_t world, int32_t* owner, int64_t* dispatch, int64_t* counts) {
    if (ne < 0 || world < 1 || (ne > 0 && (!owner || !dispatch)) || !counts) return fail(DPG_ERR_ARG, "dpg_shard_plan: bad arguments");
    std::vector<std::vector<int64_t>> disp((size_t)world);
    if (cost) {
        std::vector<int64_t> ord((size_t)ne);
        for (int64_t e = 0; e < ne; ++e) ord[(size_t)e] = e;
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return cost[a] > cost[b]; });
        std::vector<double> load((size_t)world, 0.0);
        for (int64_t e : ord) {
            int r = 0;
            for (int q = 1; q < world; ++q)
                if (load[(size_t)q] < load[(size_t)r]) r = q;
            owner[e] = r;
            load[(size_t)r] += cost[e];
            disp[(size_t)r].push_back(e);
        }
    } else {
        for (int64_t e = 0; e < ne; ++e) {
            owner[e] = (int32_t)(e % world);
            disp[(size_t)(e % world)].push_back(e);
        }
    }
    int64_t o = 0;
    for (int r = 0; r < world; ++r) {
        counts[r] = (int64_t)disp[(size_t)r].size();
        for (int64_t e : disp[(size_t)r]) dispatch[o++] = e;
    }
    return DPG_OK;
}

// The rank form's all-gathered results back in the caller's order (host only): slice r holds rank
// r's records -- its edges ascending, `slice` records of rec_bytes reserved per rank
int dpg_shard_reassemble(const int32_t* owner, int64_t ne, int32_t world, int64_t slice, int64_t rec_bytes,
                         const void* gathered, void* out) {
    if (ne < 0 || world < 1 || slice < 0 || rec_bytes <= 0 || (ne > 0 && (!owner || !gathered || !out)))
        return fail(DPG_ERR_ARG, "dpg_shard_reassemble: bad arguments");
    std::vector<int64_t> pos((size_t)world, 0);
    const char* g = static_cast<const char*>(gathered);
    char* o = static_cast<char*>(out);
    for (int64_t e = 0; e < ne; ++e) {
        const int32_t r = owner[e];
        if (r < 0 || r >= world || pos[(size_t)r] >= slice) return fail(DPG_ERR_ARG, "dpg_shard_reassemble: edge %lld owner %d out of range", (long long)e, r);
        memcpy(o + e * rec_bytes, g + (r * slice + pos[(size_t)r]++) * rec_bytes, (size_t)rec_bytes);
    }
    return DPG_OK;
}

dpg_ctx* dpg_ctx_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return no_ctx(fail(DPG_ERR_HIP, "no HIP device available"));
    if (device < 0 || device >= n) return no_ctx(fail(DPG_ERR_ARG, "device %d out of range (%d devices)", device, n));
    if (hipSetDevice(device) != hipSuccess) return no_ctx(fail(DPG_ERR_HIP, "hipSetDevice(%d) failed", device));
    dpg_ctx* c = new dpg_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own.s, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return no_ctx(fail(DPG_ERR_HIP, "hipStreamCreate failed"));
    }
    c->stream = c->own.s;
    // the side stream of the timed batch's covariance (beside the pose graph) is the context's too:
    // created with it, not inside the first solve (a stream creation costs ~7 ms on this stack)
    if (hipStreamCreateWithFlags(&c->aux.s, hipStreamNonBlocking) != hipSuccess) c->aux.s = nullptr;
    for (auto& e : c->ev) (void)e.ensure(hipEventDefault);
    dpg_gn_params_default(&c->gp);
    return c;
}

dpg_ctx* dpg_ctx_create_multi(int32_t n_gpus, const int32_t* devices) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return no_ctx(fail(DPG_ERR_HIP, "no HIP device available"));
    if (n_gpus < 1 || n_gpus > n)
        return no_ctx(fail(DPG_ERR_ARG, "dpg_ctx_create_multi: %d GPUs asked, %d present", n_gpus, n));
    std::vector<int> dl((size_t)n_gpus);
    for (int k = 0; k < n_gpus; ++k) {
        dl[(size_t)k] = devices ? devices[k] : k;
        for (int j = 0; j < k; ++j)
            if (dl[(size_t)j] == dl[(size_t)k])
                return no_ctx(fail(DPG_ERR_ARG, "dpg_ctx_create_multi: device %d listed twice", dl[(size_t)k]));
    }
    dpg_ctx* c = dpg_ctx_create(dl[0]);
    if (!c) return nullptr;
    for (int k = 1; k < n_gpus; ++k) {
        dpg_ctx* q = dpg_ctx_create(dl[(size_t)k]);
        if (!q) {
            dpg_ctx_destroy(c);
            return nullptr;
        }
        q->rank = k;
        c->peers.push_back(q);
    }
    c->comms.assign((size_t)n_gpus, nullptr);
    const ncclResult_t r = ncclCommInitAll(c->comms.data(), n_gpus, dl.data());
    if (r != ncclSuccess) {
        c->comms.clear();
        dpg_ctx_destroy(c);
        return no_ctx(fail(DPG_ERR_HIP, "ncclCommInitAll over %d devices failed: %s", n_gpus, ncclGetErrorString(r)));
    }
    c->coll = kCollRccl;
    c->world = n_gpus;
    (void)hipSetDevice(c->device);
    return c;
}

// Test / rehearsal form: k device contexts on ONE device, all on one stream (so the DAG solves of
// the k "devices" never run concurrently), the all-reduce a device-side sum in rank order.  Every
// sharded code path of the multi-device forms runs, with k > 1, on one card.
dpg_ctx* dpg_ctx_create_virtual(int32_t k, int32_t device) {
    if (k < 1 || k > kMaxVirtual)
        return no_ctx(fail(DPG_ERR_ARG, "dpg_ctx_create_virtual: %d virtual devices (1 .. %d)", k, kMaxVirtual));
    dpg_ctx* c = dpg_ctx_create(device);
    if (!c) return nullptr;
    for (int r = 1; r < k; ++r) {
        dpg_ctx* q = dpg_ctx_create(device);
        if (!q) {
            dpg_ctx_destroy(c);
            return nullptr;
        }
        q->own.release();
        q->stream = c->stream;
        q->rank = r;
        c->peers.push_back(q);
    }
    c->coll = kCollVirtual;
    c->world = k;
    return c;
}

int dpg_nccl_unique_id(void* id_out) {
    if (!id_out) return fail(DPG_ERR_ARG, "dpg_nccl_unique_id: NULL");
    static_assert(sizeof(ncclUniqueId) == DPG_NCCL_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(DPG_ERR_HIP, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    memcpy(id_out, &id, sizeof(id));
    return DPG_OK;
}

// One process per GPU (torchrun): this process's device is global rank `rank` of `world`; the
// communicator comes from the id rank 0 made (dpg_nccl_unique_id), passed around by the caller.
dpg_ctx* dpg_ctx_create_rank(int32_t device, const void* nccl_id, int32_t rank, int32_t world) {
    if (!nccl_id || world < 1 || rank < 0 || rank >= world)
        return no_ctx(fail(DPG_ERR_ARG, "dpg_ctx_create_rank: rank %d of %d", rank, world));
    dpg_ctx* c = dpg_ctx_create(device);
    if (!c) return nullptr;
    ncclUniqueId id;
    memcpy(&id, nccl_id, sizeof(id));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, world, id, rank);
    if (r != ncclSuccess) {
        dpg_ctx_destroy(c);
        return no_ctx(fail(DPG_ERR_HIP, "ncclCommInitRank(rank %d of %d) failed: %s", rank, world, ncclGetErrorString(r)));
    }
    c->comms.assign(1, comm);
    c->coll = kCollRccl;
    c->world = world;
    c->rank0 = rank;
    c->rank = rank;
    return c;
}

// One process per GPU over the caller's own collectives (blocking, host memory): a host that
// already runs a communicator (MPI, gloo), or ranks sharing one card (RCCL refuses a second rank
// on a device).  Every cross-process step of the rank form -- the cost all-reduce of the LPT plan,
// the results' all-gather, the packed system's all-reduce per Gauss-Newton iteration -- goes
// through `ops` instead of RCCL; the rest of the rank form is the same code.
dpg_ctx* dpg_ctx_create_rank_ops(int32_t device, const dpg_coll_ops* ops, int32_t rank, int32_t world) {
    if (!ops || !ops->allreduce_sum_f64 || !ops->allreduce_sum_f32 || !ops->allgather || world < 1 || rank < 0 ||
        rank >= world)
        return no_ctx(fail(DPG_ERR_ARG, "dpg_ctx_create_rank_ops: rank %d of %d (all three collectives are required)", rank, world));
    dpg_ctx* c = dpg_ctx_create(device);
    if (!c) return nullptr;
    c->host_ops = *ops;
    c->coll = kCollHost;
    c->world = world;
    c->rank0 = rank;
    c->rank = rank;
    return c;
}

int32_t dpg_ctx_num_gpus(dpg_ctx* c) { return c ? n_dev(c) : -1; }
int32_t dpg_ctx_rank(dpg_ctx* c) { return c ? c->rank0 : -1; }

// ranks of the context's collective: ncclCommCount of its communicator (RCCL forms), k (virtual),
// 1 (single device)
int32_t dpg_ctx_num_ranks(dpg_ctx* c) {
    if (!c) return -1;
    if (c->coll == kCollRccl) {
        int n = -1;
        if (ncclCommCount(c->comms[0], &n) != ncclSuccess) return fail(DPG_ERR_HIP, "ncclCommCount failed");
        return n;
    }
    return c->world;
}

void dpg_solver_options_default(dpg_solver_options* o) {
    if (!o) return;
    const dpg_chol_opts d;
    memset(o, 0, sizeof(*o));
    o->order = d.order;
    o->fused = d.fused;
    o->solve_stage = d.solve_stage;
    o->solve_maxseg = d.solve_maxseg;
    o->solve_dinv = d.solve_dinv;
    o->merge_single = d.merge_single;
    o->max_supernode_cols = d.max_supernode_cols;
    o->relax_fraction = d.relax_fraction;
    o->solve_inv_cols = d.solve_inv_cols;
}

// per context (every device of a multi-device one): applies to the next graph set up on it
int dpg_ctx_set_solver_options(dpg_ctx* c, const dpg_solver_options* o) {
    if (!c || !o || o->order < DPG_ORDER_AUTO || o->order > DPG_ORDER_ND || o->max_supernode_cols < 1 || o->solve_inv_cols < 0 ||
        !(o->relax_fraction >= 0.0))
        return fail(DPG_ERR_ARG, "bad solver options");
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_chol_opts& d = dev_ctx(c, k)->copts;
        d.order = o->order;
        d.fused = o->fused ? 1 : 0;
        d.solve_stage = o->solve_stage;
        d.solve_maxseg = o->solve_maxseg;
        d.solve_dinv = o->solve_dinv ? 1 : 0;
        d.merge_single = o->merge_single ? 1 : 0;
        d.max_supernode_cols = o->max_supernode_cols;
        d.relax_fraction = o->relax_fraction;
        d.solve_inv_cols = o->solve_inv_cols;
    }
    return DPG_OK;
}

int dpg_ctx_set_icp_schedule(dpg_ctx* c, int32_t schedule) {
    if (!c || (schedule != DPG_ICP_SCHEDULE_CALLER && schedule != DPG_ICP_SCHEDULE_MEASURED))
        return fail(DPG_ERR_ARG, "bad ICP schedule");
    c->schedule = schedule;
    return DPG_OK;
}

int dpg_ctx_set_icp_variant(dpg_ctx* c, int32_t variant) {
    if (!c || (variant != DPG_ICP_ANGULAR && variant != DPG_ICP_KDTREE && variant != DPG_ICP_GRID))
        return fail(DPG_ERR_ARG, "bad ICP variant");
    for (int k = 0; k < n_dev(c); ++k) {
        if (dev_ctx(c, k)->icp_variant != variant) dev_ctx(c, k)->idx_valid = 0;
        dev_ctx(c, k)->icp_variant = variant;
    }
    return DPG_OK;
}

int dpg_ctx_set_icp_defer_cap(dpg_ctx* c, int32_t cap) {
    if (!c || cap < 0) return fail(DPG_ERR_ARG, "bad defer cap");
    for (int k = 0; k < n_dev(c); ++k) dev_ctx(c, k)->defer_cap = cap;
    return DPG_OK;
}

int dpg_ctx_set_cov_workgroups(dpg_ctx* c, int32_t n) {
    if (!c || n < 0) return fail(DPG_ERR_ARG, "bad covariance workgroup count");
    for (int k = 0; k < n_dev(c); ++k) dev_ctx(c, k)->cov_wg = n;
    return DPG_OK;
}

int dpg_ctx_set_icp_kernel_variant(dpg_ctx* c, int32_t v) {
    if (!c || v < 0) return fail(DPG_ERR_ARG, "bad kernel variant");
    for (int k = 0; k < n_dev(c); ++k) {
        if ((dev_ctx(c, k)->kernel_variant == 2) != (v == 2)) dev_ctx(c, k)->idx_valid = 0;   // form 2: the bitonic builder
        dev_ctx(c, k)->kernel_variant = v;
    }
    return DPG_OK;
}

void dpg_ctx_adopt(dpg_ctx* c, void* child, void (*destroy)(void*)) {
    if (c && child) c->children.emplace_back(child, destroy);
}
void dpg_ctx_release_child(dpg_ctx* c, void* child) {
    if (!c) return;
    for (size_t k = 0; k < c->children.size(); ++k)
        if (c->children[k].first == child) {
            c->children.erase(c->children.begin() + (std::ptrdiff_t)k);
            return;
        }
}

// Order: children, peers, communicators, drain the stream, the collective thread, then the rest: graph, arrays,
// events and streams are members and go with the context (delete), this device current, nothing in flight.
void dpg_ctx_destroy(dpg_ctx* c) {
    if (!c) return;
    while (!c->children.empty()) {   // each child's destroy releases itself from the list
        const auto ch = c->children.back();
        ch.second(ch.first);
        if (!c->children.empty() && c->children.back().first == ch.first) c->children.pop_back();
    }
    if (c->coll == kCollVirtual) (void)hipStreamSynchronize(c->stream);   // the peers' work is on it
    for (dpg_ctx* q : c->peers) dpg_ctx_destroy(q);
    c->peers.clear();
    for (ncclComm_t m : c->comms)
        if (m) (void)ncclCommDestroy(m);
    c->comms.clear();
    (void)hipSetDevice(c->device);
    (void)join_cov(c);
    (void)hipStreamSynchronize(c->stream);
    c->hc.reset();
    if (c == g_default_ctx) g_default_ctx = nullptr;
    delete c;
}

int dpg_ctx_set_stream(dpg_ctx* c, void* s) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    if (join_cov(c)) return fail(DPG_ERR_HIP, "stream wait failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->own.release();
    c->stream = reinterpret_cast<hipStream_t>(s);
    if (c->coll == kCollVirtual)   // the virtual devices keep sharing one stream
        for (dpg_ctx* q : c->peers) q->stream = c->stream;
    return DPG_OK;
}

int dpg_ctx_synchronize(dpg_ctx* c) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    for (int k = 0; k < n_dev(c); ++k) {
        HIP_TRY(hipSetDevice(dev_ctx(c, k)->device));
        if (join_cov(dev_ctx(c, k))) return fail(DPG_ERR_HIP, "stream wait failed");
        HIP_TRY(hipStreamSynchronize(dev_ctx(c, k)->stream));
    }
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

}  // extern "C"
