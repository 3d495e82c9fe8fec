// dpg_ctx.h -- the context of the C-ABI layer, private to the HIP translation units (C++ only;
// dpg_internal.h stays the C-compatible header of the kernels and launchers).  The extern "C"
// boundary is split by subsystem over dpg_ctx.hip (context forms, options), dpg_icp_api.hip (scan
// store, batched and single ICP, covariance), dpg_gn_api.hip (pose graph, marginals) and
// dpg_sweep.hip (re-linearisation sweep, dpg_add_node); the few functions they call across each
// other are declared at the end.  The DPG store has a header of its own, dpg_dpg.h (dpg_store.hip, dpg_change.hip,
// dpg_grid.hip, dpg_loc.hip, dpg_track.hip, dpg_refine.hip; dpg_raster.h, dpg_loc_dev.h, dpg_change_plan.cpp).  Nothing here is exported from the library.
// Every device array, pinned or host-mapped block, event, stream and solver handle of the layer is a
// member that releases itself (DevBuf / PinBuf / MappedBuf, DevEvent, DevStream, CholPtr) of the
// context, its batch graph (GnGraph), its collective thread (HostColl) or a child: the release calls
// are in this header only.  Kernels and launchers take raw pointers; dpg_gn_dev is such a view.
#ifndef DPG_CTX_H
#define DPG_CTX_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/dpg_slam_c.h"
#include "dpg_buf.h"
#include "dpg_chol.h"
#include "dpg_gn_pipe.h"
#include "dpg_internal.h"

#pragma GCC visibility push(hidden)

// the thread's message for dpg_last_error; returns code
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return fail(DPG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

inline double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

// *p, or what the ABI's `def` fills in when the caller passed NULL
template <typename T>
T or_default(const T* p, void (*def)(T*)) {
    T v;
    if (p) v = *p;
    else def(&v);
    return v;
}

// The three memory kinds of OwnedBuf (dpg_buf.h): device memory, whose copy is stream-ordered and
// waited for; default-flags pinned host memory; and host-mapped coherent (fine-grained) host memory
// for the few words that a kernel and the host poll across the bus while both run.
struct DevMem {
    typedef hipStream_t stream_t;
    static int alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) != hipSuccess; }
    static void free(void* p) { (void)hipFree(p); }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess ||
               hipStreamSynchronize(s) != hipSuccess;
    }
};
struct PinMem {
    typedef hipStream_t stream_t;
    static int alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess; }
    static void free(void* p) { (void)hipHostFree(p); }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t) {
        memcpy(dst, src, bytes);
        return 0;
    }
};
struct MappedMem : PinMem {
    static int alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess; }
};
template <typename T>
using DevBuf = OwnedBuf<T, DevMem>;
template <typename T>
using PinBuf = OwnedBuf<T, PinMem>;
template <typename T>
using MappedBuf = OwnedBuf<T, MappedMem>;

// An event (a stream) that owns itself: created on first use, destroyed with its owner.  Move-only.
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept {
        std::swap(e, o.e);
        return *this;
    }
    ~DevEvent() {
        if (e) (void)hipEventDestroy(e);
    }
    int ensure(unsigned flags) { return e || hipEventCreateWithFlags(&e, flags) == hipSuccess ? 0 : -1; }
};
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { release(); }
    void release() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};
// the supernodal Cholesky's handle (dpg_chol.hip), destroyed with its owner
struct CholDestroy { void operator()(void* h) const { dpg_chol_destroy(h); } };
typedef std::unique_ptr<void, CholDestroy> CholPtr;

// The batch pose graph (dpg_gn.hip): its arrays, pinned scalars and solver, and `v`, the view of them
// that every launcher takes.  Move-assignment swaps: the moved-from object releases the previous graph.
struct GnGraph {
    dpg_gn_dev v{};
    DevBuf<dpg_factor> factors;
    DevBuf<int32_t> up_cptr, up_clist, rowptr, colidx, src_up;
    DevBuf<double> bsr, minv, poses, x, r, z, p0, p1, q, partials, scal, hb_own, scal3;
    PinBuf<double> scal3_host;
    DevBuf<uint8_t> mine;        // multi-device forms (dpg_gn_dev_set_ownership)
    DevBuf<double> hb_part;
    CholPtr chol;                // empty if the analysis failed (the PCG solver still works)
    // into an empty owner, which a failure leaves empty: host work first (pattern, lists, the Cholesky's analysis
    // and plan), then -- after hipStreamSynchronize(sync_stream) when given -- the device allocations and uploads
    int build(int64_t n_nodes, const dpg_factor* factors, int64_t n_factors, int64_t shard_begin, int64_t shard_end,
              const dpg_chol_opts* opts, hipStream_t sync_stream);
};

// Members are destroyed in reverse order of declaration, so the streams go last, after the events
// recorded on them and the buffers their work used.  Nothing is in flight by then:
// dpg_ctx_destroy drains the stream (after joining the covariance on `aux`) and stops the
// collective thread before `delete`, which is what makes every order of release safe.
struct dpg_ctx {
    int device = 0;
    DevStream own;                  // the stream made at creation, until the caller sets another
    hipStream_t stream = nullptr;   // the stream in use: own.s or the caller's
    // the batch covariance runs on `aux` beside what follows the ICP on `stream` (the pose graph
    // does not read it): ev[2] marks its end, cov_pending until `stream` has been made to wait
    DevStream aux;
    DevEvent ev[8];
    bool cov_pending = false, cov_on_aux = false;
    int32_t icp_variant = DPG_ICP_ANGULAR;
    int32_t defer_cap = 256;        // angular ICP: cooperative-queue threshold (dpg_ctx_set_icp_defer_cap)
    int32_t cov_wg = 256;           // covariance kernel workgroups beside the pose graph (dpg_ctx_set_cov_workgroups)
    int32_t kernel_variant = 0;     // angular ICP kernel form (dpg_ctx_set_icp_kernel_variant, A/B)
    float map_ms = 0.f;             // last dpg_get_map kernel (HIP events map_ev)
    DevEvent map_ev[2];             // created by the first dpg_get_map
    // scan store (batch form)
    DevBuf<float> full, ds;
    DevBuf<int64_t> ds_off_dev;
    DevBuf<int64_t> full_off_dev;  // the full clouds' offsets (the upload's device-side downsampling)
    DevBuf<float> tree_pts;        // per-node index over the downsampled clouds (k-d tree or angle order)
    DevBuf<uint16_t> tree_idx;
    DevBuf<uint16_t> buckets;      // angle variant: [V][B+1] bucket starts
    DevBuf<unsigned char> icp_scratch;   // angle variant, clouds above 4096 points: record slices
    std::vector<int64_t> full_off, ds_off;
    int64_t n_nodes = 0;
    int64_t idx_valid = 0;         // angular variant: nodes [0, idx_valid) of the store have their index
    int32_t ratio = 1;
    int32_t max_ds = 0;
    // staged edge batch
    std::vector<dpg_icp_edge> h_edges;
    DevBuf<dpg_icp_edge> edges;
    DevBuf<dpg_icp_result> res;
    DevBuf<double> hess;
    DevBuf<int32_t> trace;
    int64_t n_edges = 0;
    int32_t max_src = 0, max_tgt = 0;
    int32_t trace_iters = 0;
    dpg_icp_kparams kp{};
    bool have_cov = false;
    // single-call scratch (dpg_run_icp / icp_cov_calculate)
    DevBuf<float> s_pts;
    DevBuf<dpg_icp_edge> s_edge;
    DevBuf<dpg_icp_result> s_res;
    DevBuf<double> s_hess;
    DevBuf<int64_t> s_off;
    DevBuf<float> s_tree_pts;
    DevBuf<uint16_t> s_tree_idx;
    DevBuf<uint16_t> s_buckets;
    // pose graph
    GnGraph gn;
    bool gn_ready = false;
    dpg_gn_params gp{};
    float asm_ms = 0.f, solve_ms = 0.f;
    // node pairs (lo << 32 | hi, sorted) that share a factor of the graph set up: built from the
    // device's factor list by the first dpg_gn_marginal_pairs after a setup
    std::vector<uint64_t> gn_pairs;
    bool gn_pairs_valid = false;
    // the first pipelined GN loop's (dpg_gn_pipe.h): control block; host-mapped report slots [2] + the initial error's
    DevBuf<dpg_gn_ctl> pipe_ctl;
    MappedBuf<dpg_gn_slot> pipe_slot;
    uint32_t pipe_loop = 0;            // loops run on this device (tags their reports)
    // multi-device forms (dpg_ctx_create_multi / _rank / _virtual): this context drives local
    // device 0 and holds the batch as the caller sees it; `peers` are full single-device contexts
    // of the other local devices.  Local device k is global rank rank0 + k of `world`.
    std::vector<dpg_ctx*> peers;
    // incremental graphs and DPG stores created on this context: dpg_ctx_destroy destroys them
    // first (their buffers, helper thread and events all use the context's stream)
    std::vector<std::pair<void*, void (*)(void*)>> children;
    std::vector<ncclComm_t> comms;   // RCCL: one communicator per local device
    dpg_coll_ops host_ops{};         // kCollHost: the caller's host-memory collectives
    std::vector<double> host_hb;     // kCollHost: the packed system in host memory
    struct HostColl;                 // kCollHost, pipelined GN: the collective thread (below)
    std::unique_ptr<HostColl> hc;
    int32_t coll = 0;                // kCollNone | kCollRccl | kCollVirtual | kCollHost
    int32_t world = 1, rank0 = 0;
    int32_t rank = 0;                // global rank of THIS device context (peers too)
    // the staged batch, every form: the edges in the caller's order and their assignment --
    // batch_owner[e] = global rank aligning edge e; shard[k] = the caller indices aligned on local
    // device k, ascending (local result j of device k is edge shard[k][j])
    std::vector<dpg_icp_edge> batch;
    std::vector<int32_t> batch_owner;
    std::vector<std::vector<int64_t>> shard;
    bool batch_measured = false;     // assignment + dispatch order from measured costs
    int32_t batch_runs = 0;          // runs of the staged batch so far
    int32_t schedule = DPG_ICP_SCHEDULE_MEASURED;
    // measured alignment cost (iterations x (source + target points)) by (target, source) pair,
    // from earlier runs: the LPT assignment over ranks and the longest-first dispatch order
    std::unordered_map<uint64_t, float> cost;
    DevBuf<int32_t> shard_idx;       // per device context: its shard's caller indices
    DevBuf<float> cost_dev;          // rank form: the all-reduced cost vector of a batch
    dpg_chol_opts copts;             // solver options (dpg_ctx_set_solver_options)
    // correlative scan matching (dpg_csm.hip): pair records, rotation tables, the smoothing stencil,
    // results, and the diagnostic output (table bytes / score volume); the events around its kernel
    DevBuf<dpg_csm_pair> csm_pairs;
    DevBuf<float> csm_rot;
    DevBuf<int32_t> csm_stencil;
    DevBuf<dpg_csm_result> csm_res;
    DevBuf<int32_t> csm_diag;
    DevEvent csm_ev[2];
    bool csm_timed = false;
    // loop-closure verification (dpg_verify.hip): pair records, the counts [pair][direction][4], the
    // diagnostic table bytes; the events around its kernel
    DevBuf<dpg_verify_pair> ver_pairs;
    DevBuf<int32_t> ver_counts;
    DevBuf<uint8_t> ver_diag;
    DevEvent ver_ev[2];
    bool ver_timed = false;
};

// The rank form over the caller's collectives (kCollHost) in the pipelined Gauss-Newton loop: the
// packed system's all-reduce of iteration i runs on this thread, so the host can queue iteration
// i + 1 before iteration i's report, as over RCCL.  Per iteration, on the context stream: the
// assembly's partial system -> pinned host buffer, an event; then a one-lane kernel that waits
// until the thread has stored the iteration's tag in a host-mapped word (system-scope loads); then
// the summed system -> hb_own.  The thread waits for the event, calls the caller's all-reduce in
// place and stores the tag.  Stream order serializes the buffer's uses (the next copy into it
// follows this iteration's copy out of it).  A failed collective still stores the tag (the stream
// moves on) and sets `failed`, which the loop checks at every report.
// Owns its thread, buffers and events (dpg_gn_api.hip): create() hands out a complete object or an
// error; the destructor stops and joins the thread (its queue is empty once the context's stream
// has drained); the members then release themselves, with the context's device current.
struct dpg_ctx::HostColl {
    PinBuf<double> buf;              // pinned: the packed system, summed in place
    MappedBuf<uint32_t> flag;        // host-mapped: [0] the last tag the thread completed, [1] the wait kernel gave up (120 s)
    DevEvent ev[2];
    uint32_t next_tag = 0;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<uint32_t, hipEvent_t>> jobs;
    size_t count = 0;                // doubles of the current system
    uint64_t posted = 0, done = 0;
    bool stop = false;
    std::atomic<int> failed{0};
    static int create(const dpg_ctx* c, std::unique_ptr<HostColl>& out);
    ~HostColl();
};

enum { kCollNone = 0, kCollRccl = 1, kCollVirtual = 2, kCollHost = 3, kMaxVirtual = 16 };
inline int n_dev(const dpg_ctx* c) { return 1 + (int)c->peers.size(); }
// one process per GPU with more than one rank (dpg_ctx_create_rank / _rank_ops): the batch's
// results and costs travel between processes
inline bool is_rank_form(const dpg_ctx* c) {
    return (c->coll == kCollRccl || c->coll == kCollHost) && c->peers.empty() && c->world > 1;
}
inline dpg_ctx* dev_ctx(dpg_ctx* c, int k) { return k == 0 ? c : c->peers[(size_t)k - 1]; }
// made by dpg_ctx_create_multi / _rank / _virtual (even for one GPU: its calls then take the
// sharded paths, the all-reduce included, with one rank)
inline bool is_multi(const dpg_ctx* c) { return c->coll != kCollNone; }
// order `stream` after the last batch covariance (before anything rewrites its inputs or reads it)
inline int join_cov(dpg_ctx* c) {
    if (!c->cov_pending) return DPG_OK;
    c->cov_pending = false;
    return hipStreamWaitEvent(c->stream, c->ev[2].e, 0) == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// ---- across the layer's files ----
extern dpg_ctx* g_default_ctx;   // icp_cov_calculate / icp_cov_sandwich without a context (dpg_ctx.hip)
// dpg_icp_api.hip: the scan store back to its first V nodes; the staged batch building only the
// indexes of nodes [tree_from, n_nodes); its results in the caller's order (learn: into the cost memory)
void scans_truncate(dpg_ctx* c, int64_t V);
int icp_batch_run_from(dpg_ctx* c, int64_t tree_from);
int batch_fetch(dpg_ctx* c, dpg_icp_result* results, double* hess, bool learn);
// dpg_gn_api.hip: the Gauss-Newton loop on a set-up graph whose poses are set
int gn_loop(dpg_ctx* c, const dpg_gn_params& P, double* poses, double t0, double t1, dpg_gn_stats* st);

#pragma GCC visibility pop

#endif
