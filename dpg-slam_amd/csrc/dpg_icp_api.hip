// dpg_icp_api.hip -- the ICP half of the extern "C" boundary (include/dpg_slam_c.h,
// include/dpg_icp_cov.h): the scan store, the batched ICP (stage, run, fetch, the rank form's
// collectives), the single alignment and the covariance calls.
//
// Entry points replace (reference file:line):
//   icp_cov_calculate     -> calculate_ICP_COV            src/icp_cov/cov_func_point_to_point.h:24
//   dpg_run_icp           -> DpgSLAM::runIcp               src/dpg_slam/dpg_slam.cc:362-446
//   dpg_icp_batch_*       -> the runIcp calls of reoptimize / updatePoseGraphObsConstraints
//                            (dpg_slam.cc:85,101,263,295), batched

#include <math.h>
#include <string.h>

#include "../../include/dpg_icp_cov.h"
#include "dpg_ctx.h"

namespace {

int set_kparams(dpg_icp_kparams* kp, const dpg_icp_params* p) {
    if (!p) return fail(DPG_ERR_ARG, "params is NULL");
    if (!(p->icp_max_correspondence_distance > 0.0)) return fail(DPG_ERR_ARG, "icp_max_correspondence_distance must be > 0");
    memset(kp, 0, sizeof(*kp));
    const double r = p->icp_max_correspondence_distance;
    kp->r2 = r * r;
    float f = (float)kp->r2;
    if ((double)f > kp->r2) f = nextafterf(f, 0.0f);
    kp->r2_f = f;
    kp->h_min = (float)(r * 1.05);
    kp->eps = p->icp_maximum_transformation_epsilon;
    kp->rot_thr = 1.0 - p->icp_maximum_transformation_epsilon;
    kp->mse_abs = p->mse_threshold_absolute;
    kp->max_iter = p->icp_maximum_iterations;
    kp->min_corr = p->min_number_correspondences;
    kp->reciprocal = p->icp_use_reciprocal_correspondences ? 1 : 0;
    kp->cells_max = 4096;
    return DPG_OK;
}

int32_t round_up(int32_t v, int32_t m) { return (v + m - 1) / m * m; }

// The clouds a launch aligns and the per-node indexes (k-d trees / angle order) over them: the
// context's store, or the two clouds of a single call in its scratch.
struct ScanView {
    const float* ds;         // downsampled points
    const float* full;       // full points (covariance)
    const int64_t* ds_off;   // [n_nodes + 1] offsets into ds
    int64_t n_nodes;
    int32_t max_pts;         // largest downsampled cloud
    float* idx_pts;          // the index: points, ids, angle buckets
    uint16_t* idx_ids;
    uint16_t* buckets;
};

ScanView store_view(dpg_ctx* c) {
    return {c->ds.p, c->full.p, c->ds_off_dev.p, c->n_nodes, c->max_ds, c->tree_pts.p, c->tree_idx.p, c->buckets.p};
}

// The indexes of the nodes [tree_from, n_nodes) are built before the ICP kernel (the k-d tree and
// grid variants rebuild everything).
int launch_batch(dpg_ctx* c, const ScanView& v, const dpg_icp_edge* edges_dev, int64_t ne, dpg_icp_kparams kp,
                 int32_t max_src, int32_t max_tgt, dpg_icp_result* res_dev, double* hess_dev, int32_t* trace_dev,
                 bool timed, int64_t tree_from = 0) {
    if (c->icp_variant != DPG_ICP_ANGULAR) tree_from = 0;   // the other variants rebuild everything
    const int32_t maxp = std::max(max_src, max_tgt);
    if (maxp > 16384) return fail(DPG_ERR_SIZE, "downsampled cloud of %d points exceeds 16384", maxp);
    if (maxp > 4096 && c->icp_variant != DPG_ICP_ANGULAR)
        return fail(DPG_ERR_SIZE, "downsampled cloud of %d points: only the angular ICP variant takes more than 4096", maxp);
    int rc = join_cov(c);
    if (rc) return fail(rc, "stream wait failed");
    if (timed) HIP_TRY(hipEventRecord(c->ev[6].e, c->stream));
    if (c->icp_variant == DPG_ICP_KDTREE) {
        rc = dpg_launch_kdtree_build(v.ds, v.ds_off, v.n_nodes, v.max_pts, v.idx_pts, v.idx_ids, c->stream);
        if (rc) return fail(rc, "k-d tree build launch failed (%d)", rc);
    } else if (c->icp_variant == DPG_ICP_ANGULAR && tree_from < v.n_nodes) {
        rc = dpg_launch_angle_index(v.ds, v.ds_off + tree_from, v.n_nodes - tree_from, v.max_pts, v.idx_pts, v.idx_ids,
                                    v.buckets + tree_from * (int64_t)(dpg_angle_buckets() + 1), c->kernel_variant == 2,
                                    c->stream);
        if (rc) return fail(rc, "angle index build launch failed (%d)", rc);
    }
    if (v.ds == c->ds.p)   // the store's own indexes: current for every node now, or (other variants) overwritten
        c->idx_valid = c->icp_variant != DPG_ICP_ANGULAR ? 0 : tree_from <= c->idx_valid ? v.n_nodes : c->idx_valid;
    if (timed) HIP_TRY(hipEventRecord(c->ev[0].e, c->stream));
    if (c->icp_variant == DPG_ICP_ANGULAR) {
        kp.lds_tgt = round_up(std::max<int32_t>(maxp, 1), 16);   // record capacity
        kp.defer_cap = c->defer_cap;
        kp.kernel_variant = c->kernel_variant;
        // large clouds: a record slice per resident edge in global scratch, edges in chunks of <= 2048
        const size_t per_edge = dpg_icp_ang_scratch_per_edge(kp.lds_tgt);
        size_t sbytes = 0;
        if (per_edge) {
            sbytes = per_edge * (size_t)std::min<int64_t>(ne, 2048);
            if (c->icp_scratch.reserve(sbytes)) return fail(DPG_ERR_HIP, "out of device memory for the ICP scratch");
        }
        rc = dpg_launch_icp_ang(v.ds, v.idx_pts, v.idx_ids, v.buckets, edges_dev, ne, &kp, maxp, res_dev, trace_dev,
                                per_edge ? c->icp_scratch.p : nullptr, sbytes, c->stream);
    } else if (c->icp_variant == DPG_ICP_KDTREE) {
        kp.lds_tgt = round_up(std::max<int32_t>(maxp, 1), 64);
        rc = dpg_launch_icp_kd(v.ds, v.idx_pts, v.idx_ids, edges_dev, ne, &kp, maxp, res_dev, trace_dev, c->stream);
    } else {
        // by the larger of the two: the launcher refuses a batch whose largest cloud exceeds the
        // capacity, and a batch may hold larger sources than targets
        kp.lds_tgt = round_up(std::max<int32_t>(maxp, 1), 64);
        rc = dpg_launch_icp(v.ds, edges_dev, ne, &kp, maxp, res_dev, trace_dev, c->stream);
    }
    if (rc) return fail(rc, "ICP kernel launch failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    if (timed) HIP_TRY(hipEventRecord(c->ev[1].e, c->stream));
    if (hess_dev && timed) {   // beside the pose graph: on aux, after the ICP
        if (!c->aux.s) HIP_TRY(hipStreamCreateWithFlags(&c->aux.s, hipStreamNonBlocking));
        HIP_TRY(hipStreamWaitEvent(c->aux.s, c->ev[1].e, 0));
        rc = dpg_launch_cov(v.full, edges_dev, ne, res_dev, hess_dev, c->cov_wg, c->aux.s);
        if (rc) return fail(rc, "covariance kernel launch failed");
        HIP_TRY(hipEventRecord(c->ev[2].e, c->aux.s));
        c->cov_pending = true;
        c->cov_on_aux = true;
        return DPG_OK;
    }
    if (timed) c->cov_on_aux = false;
    if (hess_dev) {
        rc = dpg_launch_cov(v.full, edges_dev, ne, res_dev, hess_dev, 0, c->stream);
        if (rc) return fail(rc, "covariance kernel launch failed");
    }
    if (timed) HIP_TRY(hipEventRecord(c->ev[2].e, c->stream));
    return DPG_OK;
}

// ICP_COV.resize(3,3) << laser_x_variance, 0, 0, 0, laser_y_variance, ... (cov_func_point_to_point.h:572-575)
void const_cov(float vx, float vy, float vth, double cov[9]) {
    memset(cov, 0, 9 * sizeof(double));
    cov[0] = (double)vx;
    cov[4] = (double)vy;
    cov[8] = (double)vth;
}

// the context of the covariance calls made without one
dpg_ctx* ctx_or_default(dpg_ctx* c) {
    if (c) return c;
    if (!g_default_ctx) g_default_ctx = dpg_ctx_create(0);
    return g_default_ctx;
}

}  // namespace

// the scan store back to its first V nodes (dpg_add_node_pairs' rollback); the device arrays keep
// their capacity, the entries past V are overwritten by the next append
void scans_truncate(dpg_ctx* c, int64_t V) {
    if (!c) return;
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        if (V < 0 || V >= q->n_nodes) continue;
        q->full_off.resize((size_t)V + 1);
        q->ds_off.resize((size_t)V + 1);
        q->n_nodes = V;
        q->idx_valid = std::min(q->idx_valid, V);
    }
}

// R2 downsamplePointCloud of every node on the device (dpg_slam.cc:346-360, dpg_host.c
// dpg_downsample_cloud: every ratio-th point from the first, copied) -- one workgroup per node over
// the full clouds already uploaded, instead of a host pass over all of them
extern "C" __global__ void downsample_kernel(const float2* __restrict__ full, const int64_t* __restrict__ full_off,
                                  const int64_t* __restrict__ ds_off, int32_t ratio, float2* __restrict__ ds) {
    const int64_t v = blockIdx.x;
    const int64_t f0 = full_off[v], d0 = ds_off[v], nd = ds_off[v + 1] - d0;
    for (int64_t k = threadIdx.x; k < nd; k += blockDim.x) ds[d0 + k] = full[f0 + k * ratio];
}

static int scans_upload_1(dpg_ctx* c, const float* pts, const int64_t* off, int64_t V, int32_t ratio) {
    if (!c || !pts || !off || V <= 0) return fail(DPG_ERR_ARG, "dpg_scans_upload: bad arguments");
    if (ratio < 1) ratio = 1;
    HIP_TRY(hipSetDevice(c->device));
    if (c->cov_pending) {   // the store may be re-allocated under a running covariance
        HIP_TRY(hipEventSynchronize(c->ev[2].e));
        c->cov_pending = false;
    }
    const int64_t total = off[V];
    if (total >= ((int64_t)1 << 31)) return fail(DPG_ERR_SIZE, "too many points (%lld)", (long long)total);
    c->full_off.assign(off, off + V + 1);
    c->ds_off.assign((size_t)V + 1, 0);
    for (int64_t v = 0; v < V; ++v) {
        const int64_t n = off[v + 1] - off[v];
        if (n < 0) return fail(DPG_ERR_ARG, "node offsets must be non-decreasing");
        c->ds_off[(size_t)v + 1] = c->ds_off[(size_t)v] + (n + ratio - 1) / ratio;
    }
    const size_t n_ds = (size_t)(2 * std::max<int64_t>(c->ds_off[(size_t)V], 1));   // floats
    int64_t mx = 0;
    for (int64_t v = 0; v < V; ++v) mx = std::max(mx, c->ds_off[(size_t)v + 1] - c->ds_off[(size_t)v]);
    if (mx > 16384) return fail(DPG_ERR_SIZE, "a downsampled cloud has %lld points (max 16384)", (long long)mx);
    if (c->full.reserve((size_t)(2 * std::max<int64_t>(total, 1))) || c->ds.reserve(n_ds) ||
        c->ds_off_dev.reserve((size_t)V + 1) || c->full_off_dev.reserve((size_t)V + 1) || c->tree_pts.reserve(n_ds) ||
        c->tree_idx.reserve(n_ds / 2) || c->buckets.reserve((size_t)V * (size_t)(dpg_angle_buckets() + 1)))
        return fail(DPG_ERR_HIP, "out of device memory for scans");
    HIP_TRY(hipMemcpyAsync(c->full.p, pts, sizeof(float) * 2 * (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->full_off_dev.p, off, sizeof(int64_t) * ((size_t)V + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ds_off_dev.p, c->ds_off.data(), sizeof(int64_t) * ((size_t)V + 1), hipMemcpyHostToDevice,
                           c->stream));
    hipLaunchKernelGGL(downsample_kernel, dim3((unsigned)V), dim3(256), 0, c->stream, reinterpret_cast<const float2*>(c->full.p),
                       c->full_off_dev.p, c->ds_off_dev.p, ratio, reinterpret_cast<float2*>(c->ds.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_nodes = V;
    c->idx_valid = 0;
    c->ratio = ratio;
    c->max_ds = (int32_t)mx;
    return DPG_OK;
}

static int scans_append_1(dpg_ctx* c, const float* pts, const int64_t* off, int64_t k, int32_t ratio) {
    if (!c || !pts || !off || k <= 0) return fail(DPG_ERR_ARG, "dpg_scans_append: bad arguments");
    if (ratio < 1) ratio = 1;
    if (c->n_nodes == 0) return scans_upload_1(c, pts, off, k, ratio);
    if (c->cov_pending) {   // the store may be re-allocated under a running covariance
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev[2].e));
        c->cov_pending = false;
    }
    if (ratio != c->ratio) return fail(DPG_ERR_STATE, "scans were uploaded with downsample ratio %d", c->ratio);
    HIP_TRY(hipSetDevice(c->device));
    const int64_t V0 = c->n_nodes, V1 = V0 + k;
    const int64_t P0 = c->full_off[(size_t)V0], D0 = c->ds_off[(size_t)V0];
    const int64_t add = off[k] - off[0];
    if (P0 + add >= ((int64_t)1 << 31)) return fail(DPG_ERR_SIZE, "too many points");
    std::vector<int64_t> foff((size_t)k + 1), doff((size_t)k + 1);
    foff[0] = P0;
    doff[0] = D0;
    int64_t mx = c->max_ds;
    for (int64_t v = 0; v < k; ++v) {
        const int64_t n = off[v + 1] - off[v];
        if (n < 0) return fail(DPG_ERR_ARG, "node offsets must be non-decreasing");
        foff[(size_t)v + 1] = foff[(size_t)v] + n;
        doff[(size_t)v + 1] = doff[(size_t)v] + (n + ratio - 1) / ratio;
        mx = std::max(mx, (n + ratio - 1) / ratio);
    }
    if (mx > 16384) return fail(DPG_ERR_SIZE, "a downsampled cloud has %lld points (max 16384)", (long long)mx);
    const int64_t nds = doff[(size_t)k] - D0;
    std::vector<float> ds((size_t)(2 * std::max<int64_t>(nds, 1)));
    for (int64_t v = 0; v < k; ++v)
        dpg_downsample_cloud(pts + 2 * (off[v] - off[0]), off[v + 1] - off[v], ratio, ds.data() + 2 * (doff[(size_t)v] - D0));
    const size_t B = (size_t)(dpg_angle_buckets() + 1);
    if (c->full.grow((size_t)(2 * (P0 + add)), (size_t)(2 * P0), c->stream) ||
        c->ds.grow((size_t)(2 * (D0 + nds)), (size_t)(2 * D0), c->stream) ||
        c->ds_off_dev.grow((size_t)V1 + 1, (size_t)V0 + 1, c->stream) ||
        c->tree_pts.grow((size_t)(2 * (D0 + nds)), (size_t)(2 * D0), c->stream) ||
        c->tree_idx.grow((size_t)(D0 + nds), (size_t)D0, c->stream) ||
        c->buckets.grow((size_t)V1 * B, (size_t)V0 * B, c->stream))
        return fail(DPG_ERR_HIP, "out of device memory for scans");
    HIP_TRY(hipMemcpyAsync(c->full.p + 2 * P0, pts, sizeof(float) * 2 * (size_t)add, hipMemcpyHostToDevice, c->stream));
    if (nds > 0)
        HIP_TRY(hipMemcpyAsync(c->ds.p + 2 * D0, ds.data(), sizeof(float) * 2 * (size_t)nds, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ds_off_dev.p + V0 + 1, doff.data() + 1, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->full_off.insert(c->full_off.end(), foff.begin() + 1, foff.end());
    c->ds_off.insert(c->ds_off.end(), doff.begin() + 1, doff.end());
    c->n_nodes = V1;
    c->max_ds = (int32_t)mx;
    return DPG_OK;
}

// The kernel's edge records of a batch in the caller's order (R3 guesses, dpg_slam.cc:364-378;
// pad[0] = the caller's index), the kernel scalars and the largest clouds.  guesses ([ne][6]) given:
// the edges' guesses as they stand, poses unused (dpg_icp_batch_prepare_guess).
static int build_batch(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* poses, const float* guesses,
                       const dpg_icp_params* p, std::vector<dpg_icp_edge>& out, dpg_icp_kparams& kp, int32_t& ms, int32_t& mt) {
    if (!c || (!edges && ne > 0) || ne < 0 || (!poses && !guesses) || !p) return fail(DPG_ERR_ARG, "dpg_icp_batch_prepare: bad arguments");
    if (c->n_nodes <= 0) return fail(DPG_ERR_STATE, "no scans uploaded");
    if (p->downsample_icp_points_ratio != c->ratio && !(p->downsample_icp_points_ratio < 1 && c->ratio == 1))
        return fail(DPG_ERR_STATE, "scans were uploaded with downsample ratio %d", c->ratio);
    int rc = set_kparams(&kp, p);
    if (rc) return rc;
    out.resize((size_t)ne);
    ms = mt = 0;
    for (int64_t e = 0; e < ne; ++e) {
        const int32_t t = edges[2 * e], s = edges[2 * e + 1];  // node_1 = target, node_2 = source
        if (t < 0 || s < 0 || t >= c->n_nodes || s >= c->n_nodes)
            return fail(DPG_ERR_ARG, "edge %lld references a missing node", (long long)e);
        dpg_icp_edge& E = out[(size_t)e];
        memset(&E, 0, sizeof(E));
        E.src_node = s;
        E.tgt_node = t;
        E.src_ds_off = (int32_t)c->ds_off[(size_t)s];
        E.n_src_ds = (int32_t)(c->ds_off[(size_t)s + 1] - c->ds_off[(size_t)s]);
        E.tgt_ds_off = (int32_t)c->ds_off[(size_t)t];
        E.n_tgt_ds = (int32_t)(c->ds_off[(size_t)t + 1] - c->ds_off[(size_t)t]);
        E.src_full_off = (int32_t)c->full_off[(size_t)s];
        E.n_src_full = (int32_t)(c->full_off[(size_t)s + 1] - c->full_off[(size_t)s]);
        E.tgt_full_off = (int32_t)c->full_off[(size_t)t];
        E.n_tgt_full = (int32_t)(c->full_off[(size_t)t + 1] - c->full_off[(size_t)t]);
        if (guesses) memcpy(E.guess, guesses + 6 * e, sizeof(E.guess));
        else dpg_icp_guess(poses + 3 * s, poses + 3 * t, E.guess);  // R3 (dpg_slam.cc:364-378)
        E.pad[0] = (int32_t)e;
        ms = std::max(ms, E.n_src_ds);
        mt = std::max(mt, E.n_tgt_ds);
    }
    return DPG_OK;
}

constexpr size_t kCostMemoryCap = (size_t)1 << 22;   // pairs remembered (~100 MB of hash map at most)
static inline uint64_t pair_key(const dpg_icp_edge& E) { return (uint64_t)(uint32_t)E.tgt_node << 32 | (uint32_t)E.src_node; }
// what an alignment costs: its iterations, each a search over both clouds
static inline float edge_cost(const dpg_icp_edge& E, int32_t iterations) {
    return (float)std::max(iterations, 1) * (float)(E.n_src_ds + E.n_tgt_ds);
}

// device q's share of the staged batch: h = its edges in dispatch order, pad[0] = the local result
// index; every device sizes its kernel by the batch-wide largest clouds (one kernel form)
static int stage_device(dpg_ctx* q, std::vector<dpg_icp_edge>& h, const dpg_icp_kparams& kp, int32_t ms, int32_t mt,
                        const std::vector<int64_t>* idx) {
    HIP_TRY(hipSetDevice(q->device));
    int rc = join_cov(q);
    if (rc) return fail(rc, "stream wait failed");
    const size_t ne = h.size();
    if (q->edges.reserve(std::max<size_t>(ne, 1)) || q->res.reserve(std::max<size_t>(ne, 1)) ||
        q->hess.reserve(9 * std::max<size_t>(ne, 1)))
        return fail(DPG_ERR_HIP, "out of device memory for %zu edges", ne);
    if (ne > 0)
        HIP_TRY(hipMemcpyAsync(q->edges.p, h.data(), sizeof(dpg_icp_edge) * ne, hipMemcpyHostToDevice, q->stream));
    if (idx) {   // multi-device: the caller's index of every local result (dpg_gn_take_icp_measurements)
        std::vector<int32_t> ix(idx->begin(), idx->end());
        if (q->shard_idx.reserve(std::max<size_t>(ix.size(), 1))) return fail(DPG_ERR_HIP, "out of device memory");
        if (!ix.empty())
            HIP_TRY(hipMemcpyAsync(q->shard_idx.p, ix.data(), sizeof(int32_t) * ix.size(), hipMemcpyHostToDevice, q->stream));
    }
    HIP_TRY(hipStreamSynchronize(q->stream));
    q->h_edges.swap(h);
    q->kp = kp;
    q->n_edges = (int64_t)ne;
    q->max_src = ms;
    q->max_tgt = mt;
    return DPG_OK;
}

// The staged batch over the ranks and each rank's dispatch order.  measured: every edge's cost is
// known from an earlier run -- longest-processing-time assignment (longest first to the least
// loaded rank; ties: lower index, lower rank) and longest-first dispatch on every rank, so the
// alignments that bound a launch start first.  Otherwise edge e goes to rank e mod world, in the
// caller's order (the caller's lists come grouped -- successive pairs, then loop closures nearest
// first -- so every rank gets the same mix of classes).  Results keep the caller's order either way.
static int plan_and_stage(dpg_ctx* c, bool measured) {
    const int64_t ne = (int64_t)c->batch.size();
    const int W = c->world;
    std::vector<float> w;
    if (measured) {
        w.resize((size_t)ne);
        for (int64_t e = 0; e < ne; ++e) w[(size_t)e] = c->cost.at(pair_key(c->batch[(size_t)e]));
    }
    c->batch_owner.assign((size_t)ne, 0);
    std::vector<int64_t> order((size_t)std::max<int64_t>(ne, 1)), counts((size_t)W, 0);
    int rc = dpg_shard_plan(measured ? w.data() : nullptr, ne, W, c->batch_owner.data(), order.data(), counts.data());
    if (rc) return rc;
    std::vector<int64_t> first((size_t)W + 1, 0);
    for (int r = 0; r < W; ++r) first[(size_t)r + 1] = first[(size_t)r] + counts[(size_t)r];
    const int32_t ms = c->max_src, mt = c->max_tgt;
    const dpg_icp_kparams kp = c->kp;
    c->shard.assign((size_t)n_dev(c), {});
    for (int k = 0; k < n_dev(c); ++k) {
        const int r = c->rank0 + k;
        const std::vector<int64_t> d(order.begin() + first[(size_t)r], order.begin() + first[(size_t)r + 1]);
        auto& sh = c->shard[(size_t)k];
        sh = d;
        std::sort(sh.begin(), sh.end());
        std::vector<dpg_icp_edge> h(d.size());
        for (size_t q = 0; q < d.size(); ++q) {
            h[q] = c->batch[(size_t)d[q]];
            h[q].pad[0] = (int32_t)(std::lower_bound(sh.begin(), sh.end(), d[q]) - sh.begin());
        }
        if ((rc = stage_device(dev_ctx(c, k), h, kp, ms, mt, is_multi(c) ? &sh : nullptr))) return rc;
    }
    c->batch_measured = measured;
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

static bool batch_costs_known(const dpg_ctx* c) {
    for (const dpg_icp_edge& E : c->batch)
        if (c->cost.find(pair_key(E)) == c->cost.end()) return false;
    return true;
}

// one device's share of the staged batch, building the indexes of the nodes [tree_from, n_nodes)
static int batch_run_1(dpg_ctx* c, int32_t compute_cov, int32_t trace_iters, int64_t tree_from) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    dpg_icp_kparams kp = c->kp;
    int32_t* tr = nullptr;
    if (trace_iters > 0) {
        const size_t n = (size_t)c->n_edges * (size_t)trace_iters * (size_t)std::max(c->max_src, 1);
        if (c->trace.reserve(n)) return fail(DPG_ERR_HIP, "out of device memory for the trace");
        HIP_TRY(hipMemsetAsync(c->trace.p, 0xff, n * sizeof(int32_t), c->stream));
        kp.trace_iters = trace_iters;
        kp.trace_stride = std::max(c->max_src, 1);
        tr = c->trace.p;
    }
    c->trace_iters = trace_iters > 0 ? trace_iters : 0;
    c->have_cov = compute_cov != 0;
    return launch_batch(c, store_view(c), c->edges.p, c->n_edges, kp, c->max_src, c->max_tgt, c->res.p,
                        compute_cov ? c->hess.p : nullptr, tr, true, tree_from);
}

// the staged batch (single device, no covariance), building only the indexes of nodes
// [tree_from, n_nodes) (nodes appended since the last run: the others' indexes are still in place)
int icp_batch_run_from(dpg_ctx* c, int64_t tree_from) {
    ++c->batch_runs;
    return batch_run_1(c, 0, 0, tree_from);
}

// ---- the rank form's cross-process steps (blocking; every rank makes them in the same order) ----
// in-place sum of host floats over the ranks
static int coll_allreduce_f32_host(dpg_ctx* c, float* w, size_t n) {
    if (c->coll == kCollHost) {
        if (c->host_ops.allreduce_sum_f32(c->host_ops.user, w, (int64_t)n))
            return fail(DPG_ERR_HIP, "the caller's float all-reduce failed");
        return DPG_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (c->cost_dev.reserve(n)) return fail(DPG_ERR_HIP, "out of device memory");
    HIP_TRY(hipMemcpyAsync(c->cost_dev.p, w, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    const ncclResult_t nr = ncclAllReduce(c->cost_dev.p, c->cost_dev.p, n, ncclFloat, ncclSum, c->comms[0], c->stream);
    if (nr != ncclSuccess) return fail(DPG_ERR_HIP, "ncclAllReduce (costs) failed: %s", ncclGetErrorString(nr));
    HIP_TRY(hipMemcpyAsync(w, c->cost_dev.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

// every rank's `slice_bytes` (the first mine_bytes of them from local_dev, this rank's records) into
// `all` on the host, rank order
static int coll_allgather_to_host(dpg_ctx* c, const void* local_dev, size_t mine_bytes, size_t slice_bytes,
                                  std::vector<char>& all) {
    const size_t W = (size_t)c->world;
    all.assign(slice_bytes * W, 0);
    HIP_TRY(hipSetDevice(c->device));
    if (c->coll == kCollHost) {
        std::vector<char> send(slice_bytes, 0);
        if (mine_bytes) HIP_TRY(hipMemcpyAsync(send.data(), local_dev, mine_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->host_ops.allgather(c->host_ops.user, send.data(), all.data(), (int64_t)slice_bytes))
            return fail(DPG_ERR_HIP, "the caller's all-gather failed");
        return DPG_OK;
    }
    DevBuf<char> send, recv;
    if (send.reserve(slice_bytes) || recv.reserve(slice_bytes * W)) return fail(DPG_ERR_HIP, "out of device memory for the gather");
    if (mine_bytes && hipMemcpyAsync(send.p, local_dev, mine_bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
        return fail(DPG_ERR_HIP, "gather staging copy failed");
    const ncclResult_t nr = ncclAllGather(send.p, recv.p, slice_bytes, ncclChar, c->comms[0], c->stream);
    if (nr != ncclSuccess) return fail(DPG_ERR_HIP, "ncclAllGather failed: %s", ncclGetErrorString(nr));
    if (hipMemcpyAsync(all.data(), recv.p, all.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(DPG_ERR_HIP, "gather copy failed");
    return DPG_OK;
}

// device q's results (+ covariance blocks) in local order, blocking
static int fetch_local(dpg_ctx* q, size_t n, dpg_icp_result* results, double* hess) {
    HIP_TRY(hipSetDevice(q->device));
    if (join_cov(q)) return fail(DPG_ERR_HIP, "stream wait failed");
    if (results && n > 0)
        HIP_TRY(hipMemcpyAsync(results, q->res.p, sizeof(dpg_icp_result) * n, hipMemcpyDeviceToHost, q->stream));
    if (hess && n > 0)
        HIP_TRY(hipMemcpyAsync(hess, q->hess.p, sizeof(double) * 9 * n, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    return DPG_OK;
}

// the measured cost of every edge of the last run into the cost memory (blocking); on the rank form
// the ranks' costs are summed into one vector (every edge has one owner, the others add 0), so every
// rank plans the next run from the same numbers
static int harvest_costs(dpg_ctx* c) {
    const int64_t ne = (int64_t)c->batch.size();
    std::vector<float> w((size_t)std::max<int64_t>(ne, 1), 0.f);
    std::vector<dpg_icp_result> r;
    int rc;
    for (int k = 0; k < (int)c->shard.size(); ++k) {
        const auto& sh = c->shard[(size_t)k];
        if (sh.empty()) continue;
        r.resize(sh.size());
        if ((rc = fetch_local(dev_ctx(c, k), sh.size(), r.data(), nullptr))) return rc;
        for (size_t j = 0; j < sh.size(); ++j) w[(size_t)sh[j]] = edge_cost(c->batch[(size_t)sh[j]], r[j].iterations);
    }
    if (is_rank_form(c) && ne > 0 && (rc = coll_allreduce_f32_host(c, w.data(), (size_t)ne))) return rc;
    for (int64_t e = 0; e < ne; ++e)
        if (w[(size_t)e] > 0.f) c->cost[pair_key(c->batch[(size_t)e])] = w[(size_t)e];
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

// rank form: every rank's local results, gathered in equal-size slices (the largest share; each
// rank derives every other rank's share from the common plan), then put in the caller's order
static int fetch_allgather(dpg_ctx* c, void* out, size_t rec_bytes, const void* local_dev, std::vector<char>& all) {
    const int W = c->world;
    std::vector<size_t> cnt((size_t)W, 0);
    for (int32_t o : c->batch_owner) ++cnt[(size_t)o];
    const size_t slice = std::max<size_t>(*std::max_element(cnt.begin(), cnt.end()), 1);
    const size_t mine = c->shard.empty() ? 0 : c->shard[0].size();
    int rc = coll_allgather_to_host(c, local_dev, mine * rec_bytes, slice * rec_bytes, all);
    if (rc) return rc;
    return dpg_shard_reassemble(c->batch_owner.data(), (int64_t)c->batch_owner.size(), W, (int64_t)slice,
                                (int64_t)rec_bytes, all.data(), out);
}

// Results of the staged batch in the caller's order (and the covariance blocks).  On the rank form
// this is a collective: every rank receives every edge's result.  learn: the alignment costs go into
// the context's cost memory (the next plan of the same pairs); the per-node path, whose pairs are
// never re-planned, does not learn (the memory grew by every node's pairs).
int batch_fetch(dpg_ctx* c, dpg_icp_result* results, double* hess, bool learn) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    if (hess && !c->have_cov && !c->batch.empty()) return fail(DPG_ERR_STATE, "last batch ran without compute_cov");
    const int64_t ne = (int64_t)c->batch.size();
    std::vector<dpg_icp_result> own;
    dpg_icp_result* R = results;
    if (!R) {   // the costs are learnt from every fetch
        own.resize((size_t)std::max<int64_t>(ne, 1));
        R = own.data();
    }
    int rc;
    if (is_rank_form(c)) {
        std::vector<char> buf;
        if (join_cov(c)) return fail(DPG_ERR_HIP, "stream wait failed");
        if ((rc = fetch_allgather(c, R, sizeof(dpg_icp_result), c->res.p, buf))) return rc;
        if (hess && (rc = fetch_allgather(c, hess, 9 * sizeof(double), c->hess.p, buf))) return rc;
    } else {
        std::vector<dpg_icp_result> r;
        std::vector<double> h;
        for (int k = 0; k < (int)c->shard.size(); ++k) {
            const auto& ids = c->shard[(size_t)k];
            r.resize(std::max<size_t>(ids.size(), 1));
            if (hess) h.resize(9 * std::max<size_t>(ids.size(), 1));
            if ((rc = fetch_local(dev_ctx(c, k), ids.size(), r.data(), hess ? h.data() : nullptr))) return rc;
            for (size_t j = 0; j < ids.size(); ++j) {
                R[ids[j]] = r[j];
                if (hess) memcpy(hess + 9 * ids[j], h.data() + 9 * j, 9 * sizeof(double));
            }
        }
    }
    if (learn) {
        if (c->cost.size() + (size_t)ne > kCostMemoryCap) c->cost.clear();   // bounded: a long session's old pairs go
        for (int64_t e = 0; e < ne; ++e) c->cost[pair_key(c->batch[(size_t)e])] = edge_cost(c->batch[(size_t)e], R[e].iterations);
    }
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

// event pair (a, b) of the last batch: the slowest local device
static float batch_ms(dpg_ctx* c, int a, int b) {
    float worst = -1.f;
    for (int k = 0; k < (c ? n_dev(c) : 0); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        float ms = -1.f;
        if (hipSetDevice(q->device) != hipSuccess || hipEventSynchronize(q->ev[b].e) != hipSuccess ||
            hipEventElapsedTime(&ms, q->ev[a].e, q->ev[b].e) != hipSuccess)
            return -1.f;
        worst = std::max(worst, ms);
    }
    if (c) (void)hipSetDevice(c->device);
    return worst;
}

// the last launch on device q, from its own records: sum over its edges of iterations x (8N + 8M + 8N)
static double batch_bytes_1(dpg_ctx* c) {
    if (!c || c->n_edges <= 0) return 0.0;
    std::vector<dpg_icp_result> r((size_t)c->n_edges);
    if (hipMemcpy(r.data(), c->res.p, sizeof(dpg_icp_result) * r.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    double bytes = 0.0;
    for (int64_t e = 0; e < c->n_edges; ++e) {
        const dpg_icp_edge& E = c->h_edges[(size_t)e];   // dispatch order; its result is r[E.pad[0]]
        // correspondence kernel per edge-iteration: 8N (source xy) + 8M (target xy) + 8N (idx + d^2)
        bytes += (double)r[(size_t)E.pad[0]].iterations * (16.0 * E.n_src_ds + 8.0 * E.n_tgt_ds);
    }
    return bytes;
}

extern "C" {

// every device of a multi-GPU context holds every scan (5000 x 1000 points: 40 MB of downsampled
// clouds per device), so any edge can be aligned on any device
int dpg_scans_upload(dpg_ctx* c, const float* pts, const int64_t* off, int64_t V, int32_t ratio) {
    if (!c) return fail(DPG_ERR_ARG, "dpg_scans_upload: bad arguments");
    c->cost.clear();   // a new store: node ids name other scans
    for (int k = 0; k < n_dev(c); ++k) {
        const int rc = scans_upload_1(dev_ctx(c, k), pts, off, V, ratio);
        if (rc) return rc;
    }
    return hipSetDevice(c->device) == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

int dpg_scans_append(dpg_ctx* c, const float* pts, const int64_t* off, int64_t k, int32_t ratio) {
    if (!c) return fail(DPG_ERR_ARG, "dpg_scans_append: bad arguments");
    for (int d = 0; d < n_dev(c); ++d) {
        const int rc = scans_append_1(dev_ctx(c, d), pts, off, k, ratio);
        if (rc) return rc;
    }
    return hipSetDevice(c->device) == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// The scan store as host copies (the graph checkpoint, dpg_inc_save): node count, downsample
// ratio, and -- when the arrays are given -- the node offsets [n + 1] and the full clouds [off[n]][2]
int dpg_scans_export(dpg_ctx* c, int64_t* n_nodes, int32_t* ratio, int64_t* off, float* pts) {
    if (!c || !n_nodes || !ratio) return fail(DPG_ERR_ARG, "dpg_scans_export: bad arguments");
    *n_nodes = c->n_nodes;
    *ratio = c->ratio;
    if (c->n_nodes <= 0) return DPG_OK;
    if (off) std::copy(c->full_off.begin(), c->full_off.begin() + c->n_nodes + 1, off);
    if (pts) {
        HIP_TRY(hipSetDevice(c->device));
        const size_t total = (size_t)c->full_off[(size_t)c->n_nodes];
        if (total) HIP_TRY(hipMemcpyAsync(pts, c->full.p, sizeof(float) * 2 * total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return DPG_OK;
}

// The neighbour index of every stored node (the incremental path builds it node by node as nodes
// arrive; a store restored from a checkpoint needs all of it before its next dpg_add_node)
int dpg_scans_index_all(dpg_ctx* c) {
    if (!c) return fail(DPG_ERR_ARG, "dpg_scans_index_all: ctx is NULL");
    if (c->n_nodes <= 0 || c->icp_variant != DPG_ICP_ANGULAR) return DPG_OK;   // the other variants index per batch
    HIP_TRY(hipSetDevice(c->device));
    const int rc = dpg_launch_angle_index(c->ds.p, c->ds_off_dev.p, c->n_nodes, c->max_ds, c->tree_pts.p, c->tree_idx.p,
                                          c->buckets.p, c->kernel_variant == 2, c->stream);
    if (rc) return fail(rc, "angle index build failed");
    c->idx_valid = c->n_nodes;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

// Stage an edge batch on every device.  The assignment uses measured costs when every edge of the
// batch has been aligned before (a sweep re-aligns the previous sweep's pairs from similar guesses).
static int batch_prepare(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* poses, const float* guesses,
                         const dpg_icp_params* p) {
    if (!c) return fail(DPG_ERR_ARG, "dpg_icp_batch_prepare: bad arguments");
    int32_t ms = 0, mt = 0;
    dpg_icp_kparams kp;
    std::vector<dpg_icp_edge> all;
    int rc = build_batch(c, edges, ne, poses, guesses, p, all, kp, ms, mt);
    if (rc) return rc;
    c->batch.swap(all);
    c->kp = kp;
    c->max_src = ms;
    c->max_tgt = mt;
    c->batch_runs = 0;
    return plan_and_stage(c, c->schedule == DPG_ICP_SCHEDULE_MEASURED && ne > 0 && batch_costs_known(c));
}

int dpg_icp_batch_prepare(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* poses, const dpg_icp_params* p) {
    if (!poses) return fail(DPG_ERR_ARG, "dpg_icp_batch_prepare: bad arguments");
    return batch_prepare(c, edges, ne, poses, nullptr, p);
}

// the same with every edge's guess given (a scan matcher's refined guesses, dpg_csm_batch)
int dpg_icp_batch_prepare_guess(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* guesses,
                                const dpg_icp_params* p) {
    if (!guesses) return fail(DPG_ERR_ARG, "dpg_icp_batch_prepare_guess: guesses is NULL");
    return batch_prepare(c, edges, ne, nullptr, guesses, p);
}

// Run the staged batch on every device (launches only: the devices run concurrently).  A batch
// run again after its first run (the bench's steps) is re-planned once from its measured costs.
int dpg_icp_batch_run(dpg_ctx* c, int32_t compute_cov, int32_t trace_iters) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    if (trace_iters > 0 && is_multi(c)) return fail(DPG_ERR_STATE, "the correspondence trace is a single-device diagnostic");
    int rc;
    if (c->schedule == DPG_ICP_SCHEDULE_MEASURED && !c->batch_measured && c->batch_runs > 0 && trace_iters <= 0 &&
        !c->batch.empty()) {
        if (!batch_costs_known(c) && (rc = harvest_costs(c))) return rc;
        if (batch_costs_known(c) && (rc = plan_and_stage(c, true))) return rc;
    }
    // the angle index is a function of the stored scans alone: a batch run again on the same store
    // (the next sweep, the bench's steps) reuses it and builds only the nodes appended since
    for (int k = 0; k < n_dev(c); ++k) {
        dpg_ctx* q = dev_ctx(c, k);
        if ((rc = batch_run_1(q, compute_cov, trace_iters, std::min(q->idx_valid, q->n_nodes)))) return rc;
    }
    c->have_cov = compute_cov != 0;
    ++c->batch_runs;
    HIP_TRY(hipSetDevice(c->device));
    return DPG_OK;
}

float dpg_kdtree_build_ms(dpg_ctx* c) {
    float ms = -1.f;
    if (!c || hipEventSynchronize(c->ev[0].e) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->ev[6].e, c->ev[0].e) != hipSuccess) return -1.f;
    return ms;
}

int dpg_icp_batch_fetch(dpg_ctx* c, dpg_icp_result* results, double* hess, int64_t cap) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    if ((results || hess) && cap < (int64_t)c->batch.size())
        return fail(DPG_ERR_SIZE, "result buffers hold fewer records than the staged batch (dpg_icp_batch_size)");
    return batch_fetch(c, results, hess, true);
}

// edges of the staged batch (dpg_icp_batch_prepare's, or the one a sweep / dpg_add_node staged):
// what dpg_icp_batch_fetch writes
int64_t dpg_icp_batch_size(dpg_ctx* c) { return c ? (int64_t)c->batch.size() : fail(DPG_ERR_ARG, "ctx is NULL"); }

int dpg_icp_batch_fetch_trace(dpg_ctx* c, int32_t* trace, int64_t trace_cap, int64_t* max_src_out) {
    if (!c) return fail(DPG_ERR_ARG, "ctx is NULL");
    if (is_multi(c)) return fail(DPG_ERR_STATE, "the correspondence trace is a single-device diagnostic");
    if (max_src_out) *max_src_out = std::max(c->max_src, 1);
    if (!trace) return DPG_OK;
    if (c->trace_iters <= 0) return fail(DPG_ERR_STATE, "last batch ran without a trace");
    const size_t n = (size_t)c->n_edges * (size_t)c->trace_iters * (size_t)std::max(c->max_src, 1);
    if (trace_cap < 0 || (size_t)trace_cap < n) return fail(DPG_ERR_SIZE, "trace buffer smaller than E * trace_iters * max_src");
    HIP_TRY(hipMemcpyAsync(trace, c->trace.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

float dpg_icp_batch_kernel_ms(dpg_ctx* c) { return batch_ms(c, 0, 1); }

float dpg_cov_batch_kernel_ms(dpg_ctx* c) { return batch_ms(c, 1, 2); }

int32_t dpg_cov_batch_overlapped(dpg_ctx* c) { return c && c->cov_on_aux ? 1 : 0; }

// the local devices' launches (the rank form: this rank's share)
double dpg_icp_batch_algorithmic_bytes(dpg_ctx* c) {
    if (!c) return 0.0;
    double b = 0.0;
    for (int k = 0; k < n_dev(c); ++k) {
        (void)hipSetDevice(dev_ctx(c, k)->device);
        const double x = batch_bytes_1(dev_ctx(c, k));
        if (x < 0) return x;
        b += x;
    }
    (void)hipSetDevice(c->device);
    return b;
}

// ------------------------------------------------------------------ single alignment / covariance
int dpg_run_icp(dpg_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float pose_src[3],
                const float pose_tgt[3], const dpg_icp_params* p, dpg_icp_result* result, double cov_out[9],
                double hess_out[9]) {
    if (!c || !src || !tgt || ns < 0 || nt < 0 || !pose_src || !pose_tgt || !p || !result)
        return fail(DPG_ERR_ARG, "dpg_run_icp: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    dpg_icp_kparams kp;
    int rc = set_kparams(&kp, p);
    if (rc) return rc;
    const int32_t ratio = p->downsample_icp_points_ratio > 0 ? p->downsample_icp_points_ratio : 1;
    const int64_t nsd = (ns + ratio - 1) / ratio, ntd = (nt + ratio - 1) / ratio;
    // layout: [src full | tgt full | src ds | tgt ds]
    std::vector<float> buf((size_t)(2 * (ns + nt + nsd + ntd) + 2));
    memcpy(buf.data(), src, sizeof(float) * 2 * (size_t)ns);
    memcpy(buf.data() + 2 * ns, tgt, sizeof(float) * 2 * (size_t)nt);
    dpg_downsample_cloud(src, ns, ratio, buf.data() + 2 * (ns + nt));
    dpg_downsample_cloud(tgt, nt, ratio, buf.data() + 2 * (ns + nt + nsd));
    dpg_icp_edge E;
    memset(&E, 0, sizeof(E));
    E.src_node = 0;
    E.tgt_node = 1;
    E.src_full_off = 0; E.n_src_full = (int32_t)ns;
    E.tgt_full_off = (int32_t)ns; E.n_tgt_full = (int32_t)nt;
    // downsampled clouds (and their trees) are addressed relative to the ds part of the buffer
    E.src_ds_off = 0; E.n_src_ds = (int32_t)nsd;
    E.tgt_ds_off = (int32_t)nsd; E.n_tgt_ds = (int32_t)ntd;
    dpg_icp_guess(pose_src, pose_tgt, E.guess);
    const int64_t offs[3] = {0, nsd, nsd + ntd};
    if (c->s_pts.reserve(buf.size()) || c->s_edge.reserve(1) || c->s_res.reserve(1) || c->s_hess.reserve(9) ||
        c->s_off.reserve(3) || c->s_tree_pts.reserve((size_t)(2 * (nsd + ntd) + 2)) ||
        c->s_tree_idx.reserve((size_t)(nsd + ntd + 1)) || c->s_buckets.reserve((size_t)(2 * (dpg_angle_buckets() + 1))))
        return fail(DPG_ERR_HIP, "out of device memory");
    HIP_TRY(hipMemcpyAsync(c->s_pts.p, buf.data(), sizeof(float) * buf.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->s_edge.p, &E, sizeof(E), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->s_off.p, offs, sizeof(offs), hipMemcpyHostToDevice, c->stream));
    const ScanView two{c->s_pts.p + 2 * (ns + nt), c->s_pts.p, c->s_off.p, 2, (int32_t)std::max(nsd, ntd),
                       c->s_tree_pts.p, c->s_tree_idx.p, c->s_buckets.p};
    rc = launch_batch(c, two, c->s_edge.p, 1, kp, (int32_t)nsd, (int32_t)ntd, c->s_res.p,
                      hess_out ? c->s_hess.p : nullptr, nullptr, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(result, c->s_res.p, sizeof(dpg_icp_result), hipMemcpyDeviceToHost, c->stream));
    if (hess_out) HIP_TRY(hipMemcpyAsync(hess_out, c->s_hess.p, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (cov_out) const_cov(p->laser_x_variance, p->laser_y_variance, p->laser_theta_variance, cov_out);
    return DPG_OK;
}

int icp_cov_calculate(dpg_ctx* c, const float* data, int64_t nd, const float* model, int64_t nm, const float T[16],
                      float vx, float vy, float vth, double cov_out[9], double hess_out[9]) {
    if (!cov_out || !T) return fail(DPG_ERR_ARG, "icp_cov_calculate: bad arguments");
    const_cov(vx, vy, vth, cov_out);
    if (!hess_out) return DPG_OK;
    if (!data || !model || nd < 0 || nm < 0) return fail(DPG_ERR_ARG, "icp_cov_calculate: bad clouds");
    if (!(c = ctx_or_default(c))) return DPG_ERR_HIP;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> buf((size_t)(2 * (nd + nm) + 2));
    memcpy(buf.data(), data, sizeof(float) * 2 * (size_t)nd);
    memcpy(buf.data() + 2 * nd, model, sizeof(float) * 2 * (size_t)nm);
    dpg_icp_edge E;
    memset(&E, 0, sizeof(E));
    E.src_full_off = 0; E.n_src_full = (int32_t)nd;
    E.tgt_full_off = (int32_t)nd; E.n_tgt_full = (int32_t)nm;
    dpg_icp_result R;
    memset(&R, 0, sizeof(R));
    R.T[0] = T[0]; R.T[1] = T[1]; R.T[2] = T[3];    // row-major 4x4 -> rows (T00 T01 T03 / T10 T11 T13)
    R.T[3] = T[4]; R.T[4] = T[5]; R.T[5] = T[7];
    if (c->s_pts.reserve(buf.size()) || c->s_edge.reserve(1) || c->s_res.reserve(1) || c->s_hess.reserve(9))
        return fail(DPG_ERR_HIP, "out of device memory");
    HIP_TRY(hipMemcpyAsync(c->s_pts.p, buf.data(), sizeof(float) * buf.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->s_edge.p, &E, sizeof(E), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->s_res.p, &R, sizeof(R), hipMemcpyHostToDevice, c->stream));
    int rc = dpg_launch_cov(c->s_pts.p, c->s_edge.p, 1, c->s_res.p, c->s_hess.p, 0, c->stream);
    if (rc) return fail(rc, "covariance kernel launch failed");
    HIP_TRY(hipMemcpyAsync(hess_out, c->s_hess.p, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

int icp_cov_sandwich(dpg_ctx* c, const float* data, int64_t nd, const float* model, int64_t nm, const float T[16],
                     double cov6_out[36], double cov3_out[9]) {
    if (!T || !data || !model || nd < 1 || nm < 1 || nd > INT32_MAX / 4 || nm > INT32_MAX / 4)
        return fail(DPG_ERR_ARG, "icp_cov_sandwich: bad arguments");
    // the closed forms hold at the planar operating point z = pitch = roll = 0 (the reference reads
    // z, roll, pitch from T's third row, cov_func_point_to_point.h:26-31): a non-planar T is refused
    // rather than silently evaluated at the wrong point
    if (T[2] != 0.f || T[6] != 0.f || T[8] != 0.f || T[9] != 0.f || T[10] != 1.f || T[11] != 0.f)
        return fail(DPG_ERR_ARG, "icp_cov_sandwich: T is not planar (needs T20 = T21 = T02 = T12 = T23 = 0, T22 = 1)");
    if (!(c = ctx_or_default(c))) return DPG_ERR_HIP;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> buf((size_t)(2 * (nd + nm)) + 8);
    memcpy(buf.data(), data, sizeof(float) * 2 * (size_t)nd);
    memcpy(buf.data() + 2 * nd, model, sizeof(float) * 2 * (size_t)nm);
    float* T6 = buf.data() + 2 * (nd + nm);   // rows (T00 T01 T03 / T10 T11 T13), as the ICP result keeps them
    T6[0] = T[0]; T6[1] = T[1]; T6[2] = T[3]; T6[3] = T[4]; T6[4] = T[5]; T6[5] = T[7];
    if (c->s_pts.reserve(buf.size()) || c->s_hess.reserve(16)) return fail(DPG_ERR_HIP, "out of device memory");
    HIP_TRY(hipMemcpyAsync(c->s_pts.p, buf.data(), sizeof(float) * buf.size(), hipMemcpyHostToDevice, c->stream));
    int rc = dpg_launch_cov6(c->s_pts.p, (int32_t)nd, (int32_t)nm, c->s_pts.p + 2 * (nd + nm), c->s_hess.p, c->stream);
    if (rc) return fail(rc, "covariance kernel launch failed");
    double sm[16];
    HIP_TRY(hipMemcpyAsync(sm, c->s_hess.p, sizeof(sm), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t nh = std::min(nd, nm), nb = std::min<int64_t>(nh, 200);
    double cov6[36];
    if ((rc = dpg_cov6_from_sums(sm, nh, nb, cov6))) return fail(rc, "icp_cov_sandwich: d2J_dX2 is singular");
    if (cov6_out) memcpy(cov6_out, cov6, sizeof(cov6));
    if (cov3_out) {
        const int ix[3] = {0, 1, 3};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) cov3_out[3 * i + j] = cov6[6 * ix[i] + ix[j]];
    }
    return DPG_OK;
}

}  // extern "C"
