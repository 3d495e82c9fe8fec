// dpg_sweep.hip -- the sweep half of the extern "C" boundary (include/dpg_slam_c.h): loop-closure
// candidates, the map, the re-linearisation sweep on the batch graph and on the incremental one
// (DpgSLAM::reoptimize, dpg_slam.cc:35-119), and the per-node update (dpg_add_node;
// updatePoseGraphObsConstraints, dpg_slam.cc:255-314).

#include <math.h>
#include <string.h>

#include "dpg_ctx.h"

// candidate pairs on the GPU (dpg_reopt.hip): count per node, host prefix sum, write
static int64_t lc_candidates(dpg_ctx* c, int64_t V, const int32_t* pass, const float* est, float within,
                             float across, std::vector<int32_t>& pairs) {
    DevBuf<float> dposes;
    DevBuf<int32_t> dpass, dcount, dpairs;
    DevBuf<int64_t> doff;
    if (dposes.reserve((size_t)(3 * V)) || dpass.reserve((size_t)V) || dcount.reserve((size_t)V) ||
        doff.reserve((size_t)V))
        return fail(DPG_ERR_HIP, "allocation failed");
    int64_t acc = 0;
    std::vector<int32_t> cnt((size_t)V);
    std::vector<int64_t> off((size_t)V);
    const auto search = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(dposes.p, est, sizeof(float) * 3 * V, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dpass.p, pass, sizeof(int32_t) * V, hipMemcpyHostToDevice, c->stream));
        if (dpg_launch_lc_count(dposes.p, dpass.p, V, within, across, dcount.p, c->stream)) return DPG_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(cnt.data(), dcount.p, sizeof(int32_t) * V, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < V; ++i) { off[(size_t)i] = acc; acc += cnt[(size_t)i]; }
        pairs.assign((size_t)(2 * acc), 0);
        if (acc == 0) return DPG_OK;
        if (dpairs.reserve((size_t)(2 * acc))) return DPG_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * V, hipMemcpyHostToDevice, c->stream));
        if (dpg_launch_lc_write(dposes.p, dpass.p, V, within, across, doff.p, dpairs.p, c->stream)) return DPG_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(pairs.data(), dpairs.p, sizeof(int32_t) * 2 * acc, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return DPG_OK;
    };
    if (search()) return fail(DPG_ERR_HIP, "loop-closure candidate search failed: %s", hipGetErrorString(hipGetLastError()));
    return acc;
}

// The sweep of DpgSLAM::reoptimize up to the alignments (dpg_slam.cc:35-107): candidates, the ICP
// edge list (successive, then candidates), the factor list (per node a pass prior or the odometry
// Between, then one Between slot per ICP edge, first at first_icp) and ONE batched ICP launched on
// the context's stream, then its results (the caller may fetch them again: the batch stays staged).
namespace {
struct Sweep {
    dpg_icp_params I;
    dpg_reopt_params R;
    dpg_reopt_stats S;
    std::vector<int32_t> edges;        // [E][2], E = S.n_icp_edges: n_succ successive pairs, then the candidates
    std::vector<dpg_factor> F;
    std::vector<dpg_icp_result> res;   // [E]
    int64_t first_icp = 0, n_succ = 0;
    double t1 = 0.0, t2 = 0.0;         // host clock: candidates found, alignments fetched
};
}  // namespace

static int reopt_sweep(dpg_ctx* c, int64_t V, const int32_t* pass, const float* est, const float* odom,
                       const dpg_icp_params* ip, const dpg_reopt_params* rp, Sweep& w) {
    if (c->n_nodes != V) return fail(DPG_ERR_STATE, "scans of %lld nodes uploaded, sweep over %lld",
                                     (long long)c->n_nodes, (long long)V);
    w.I = or_default(ip, dpg_icp_params_default);
    w.R = or_default(rp, dpg_reopt_params_default);
    const dpg_reopt_params& R = w.R;
    std::vector<int32_t>& edges = w.edges;
    std::vector<dpg_factor>& F = w.F;
    memset(&w.S, 0, sizeof(w.S));
    const double t0 = now_ms();
    // 1. loop-closure candidates (dpg_slam.cc:91-98)
    std::vector<int32_t> lc;
    const int64_t K = lc_candidates(c, V, pass, est, R.max_node_dist_within_pass, R.max_node_dist_across_passes, lc);
    if (K < 0) return (int)K;
    w.t1 = now_ms();
    // 2. ICP edges: successive (i-1, i), then the candidates (j, i) -- {node_1 target, node_2 source}
    w.n_succ = V - 1;
    const int64_t E = w.n_succ + K;
    edges.assign((size_t)(2 * E), 0);
    for (int64_t i = 1; i < V; ++i) { edges[(size_t)(2 * (i - 1))] = (int32_t)(i - 1); edges[(size_t)(2 * (i - 1) + 1)] = (int32_t)i; }
    if (K > 0) memcpy(edges.data() + 2 * w.n_succ, lc.data(), sizeof(int32_t) * 2 * (size_t)K);
    // 3. factors: per node a prior (new pass) or the odometry Between (dpg_slam.cc:40-79), then one
    //    slot per ICP edge (measurements filled on device after the batch)
    F.clear();
    F.reserve((size_t)(V + E));
    int32_t cur_pass = -1;
    for (int64_t i = 0; i < V; ++i) {
        if (i == 0 || pass[i] != cur_pass) {
            dpg_factor f;
            memset(&f, 0, sizeof(f));
            f.kind = DPG_FACTOR_PRIOR;
            f.i = (int32_t)i;
            for (int k = 0; k < 3; ++k) {
                const double sd = (double)R.new_pass_std_dev[k];
                f.info[k] = 1.0 / (sd * sd);
            }
            F.push_back(f);
            cur_pass = pass[i];
        } else if (R.odometry_constraints) {
            dpg_factor f;
            const int rc = dpg_odometry_factor(odom + 3 * (i - 1), odom + 3 * i, (int32_t)(i - 1), (int32_t)i,
                                               R.motion_model[0], R.motion_model[1], R.motion_model[2],
                                               R.motion_model[3], &f);
            if (rc) return fail(rc, "odometry factor %lld has no motion (zero sigma)", (long long)i);
            F.push_back(f);
        }
    }
    w.first_icp = (int64_t)F.size();
    for (int64_t e = 0; e < E; ++e) {
        dpg_factor f;
        memset(&f, 0, sizeof(f));
        f.kind = DPG_FACTOR_BETWEEN;
        f.i = edges[(size_t)(2 * e)];
        f.j = edges[(size_t)(2 * e + 1)];
        F.push_back(f);
    }
    // 4. one batched ICP of every edge from the estimated poses (runIcp, dpg_slam.cc:362-446)
    int rc = dpg_icp_batch_prepare(c, edges.data(), E, est, &w.I);
    if (!rc) rc = dpg_icp_batch_run(c, 0, 0);
    w.S.n_candidates = K;
    w.S.n_icp_edges = E;
    w.S.ms_candidates = w.t1 - t0;
    if (rc) return rc;
    // the alignments end here
    w.res.resize((size_t)std::max<int64_t>(E, 1));
    if ((rc = dpg_icp_batch_fetch(c, w.res.data(), nullptr, (int64_t)w.res.size()))) return rc;
    w.t2 = now_ms();
    return DPG_OK;
}

// Which alignments become factors (addObservationConstraint, dpg_slam.cc:85-104, 263-301): the
// first n_succ (successive pairs) always, a loop closure when its alignment converged.  A failed
// kernel self-check (DPG_ICP_INTERNAL) on any edge is an error, never a factor, and is found
// before anything is appended.
static bool closure_ok(const dpg_icp_result& r) { return r.converged && r.status == DPG_ICP_OK; }

static int append_icp_factors(const char* fn, const dpg_icp_result* res, const std::vector<int32_t>& edges, int64_t n_succ,
                              const dpg_icp_params& I, std::vector<dpg_factor>& F, int64_t& n_loop_closures) {
    const int64_t E = (int64_t)edges.size() / 2;
    for (int64_t e = 0; e < E; ++e)
        if (res[e].status == DPG_ICP_INTERNAL)
            return fail(DPG_ERR_INTERNAL, "%s: alignment %lld failed its internal check", fn, (long long)e);
    for (int64_t e = 0; e < E; ++e) {
        if (e >= n_succ && !closure_ok(res[e])) continue;
        dpg_factor f;
        dpg_icp_factor(&res[e], edges[(size_t)(2 * e)], edges[(size_t)(2 * e + 1)], &I, &f);
        F.push_back(f);
        if (e >= n_succ) ++n_loop_closures;
    }
    return DPG_OK;
}

extern "C" {

void dpg_reopt_params_default(dpg_reopt_params* p) {
    if (!p) return;
    p->max_node_dist_within_pass = 5.0f;
    p->max_node_dist_across_passes = 2.0f;
    p->new_pass_std_dev[0] = 0.2f;
    p->new_pass_std_dev[1] = 0.2f;
    p->new_pass_std_dev[2] = 0.15f;
    for (int k = 0; k < 4; ++k) p->motion_model[k] = 0.4f;
    p->odometry_constraints = 1;
}

int64_t dpg_loop_closure_candidates(dpg_ctx* c, int64_t V, const int32_t* pass, const float* est, float within,
                                    float across, int32_t* pairs_out, int64_t cap) {
    if (!c || V < 0 || (V > 0 && (!pass || !est))) return fail(DPG_ERR_ARG, "bad arguments");
    std::vector<int32_t> pairs;
    const int64_t K = lc_candidates(c, V, pass, est, within, across, pairs);
    if (K < 0) return K;
    if (pairs_out && cap > 0) memcpy(pairs_out, pairs.data(), sizeof(int32_t) * 2 * (size_t)std::min(K, cap));
    return K;
}

int64_t dpg_get_map(dpg_ctx* c, const float* est, int32_t fraction, float* out, int64_t cap) {
    if (!c || !est || fraction <= 0) return fail(DPG_ERR_ARG, "bad arguments");
    const int64_t V = c->n_nodes;
    if (V <= 0 || (int64_t)c->full_off.size() != V + 1) return fail(DPG_ERR_STATE, "no scans uploaded");
    const int64_t P = c->full_off[(size_t)V];
    const int64_t K = (P + fraction - 1) / fraction;
    if (!out || cap <= 0 || K == 0) return K;
    // Rotation2Df(angle): cosf/sinf on the host, as the reference evaluates them
    std::vector<float> fr((size_t)(4 * V));
    for (int64_t v = 0; v < V; ++v) {
        fr[(size_t)(4 * v)] = est[3 * v];
        fr[(size_t)(4 * v + 1)] = est[3 * v + 1];
        fr[(size_t)(4 * v + 2)] = cosf(est[3 * v + 2]);
        fr[(size_t)(4 * v + 3)] = sinf(est[3 * v + 2]);
    }
    DevBuf<float> dfr, dout;
    DevBuf<int64_t> doff;
    const auto assemble = [&]() -> int {
        if (dfr.reserve((size_t)(4 * V)) || dout.reserve((size_t)(2 * K)) || doff.reserve((size_t)(V + 1))) return DPG_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(dfr.p, fr.data(), sizeof(float) * 4 * V, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(doff.p, c->full_off.data(), sizeof(int64_t) * (V + 1), hipMemcpyHostToDevice, c->stream));
        if (c->map_ev[0].ensure(hipEventDefault) || c->map_ev[1].ensure(hipEventDefault)) return DPG_ERR_HIP;
        HIP_TRY(hipEventRecord(c->map_ev[0].e, c->stream));
        if (dpg_launch_map_points(c->full.p, doff.p, dfr.p, V, fraction, dout.p, c->stream)) return DPG_ERR_HIP;
        HIP_TRY(hipEventRecord(c->map_ev[1].e, c->stream));
        HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(float) * 2 * std::min(K, cap), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->map_ev[0].e, c->map_ev[1].e) == hipSuccess) c->map_ms = ms;
        return DPG_OK;
    };
    if (assemble()) return fail(DPG_ERR_HIP, "map assembly failed: %s", hipGetErrorString(hipGetLastError()));
    return K;
}

float dpg_get_map_kernel_ms(dpg_ctx* c) { return c ? c->map_ms : -1.f; }

int dpg_reoptimize(dpg_ctx* c, int64_t V, const int32_t* pass, const float* est, const float* odom,
                   const dpg_icp_params* ip, const dpg_gn_params* gp, const dpg_reopt_params* rp, double* poses_out,
                   dpg_reopt_stats* st) {
    if (!c || V <= 0 || !pass || !est || !odom || !poses_out) return fail(DPG_ERR_ARG, "bad arguments");
    const dpg_gn_params P = or_default(gp, dpg_gn_params_default);
    Sweep w;
    int rc = reopt_sweep(c, V, pass, est, odom, ip, rp, w);
    if (rc) return rc;
    dpg_reopt_stats& S = w.S;
    const int64_t E = S.n_icp_edges;
    // 5. batch Gauss-Newton from the estimated poses (optimizeGraph, dpg_slam.cc:111-119, 316-329);
    //    the ICP slots take the results where they were aligned (multi-device: on each device), and
    //    their outcomes give the loop-closure count
    if ((rc = dpg_gn_setup(c, V, w.F.data(), (int64_t)w.F.size(), 0, (int64_t)w.F.size(), &P))) return rc;
    if ((rc = dpg_gn_take_icp_measurements(c, w.first_icp, E, w.n_succ, &w.I))) return rc;
    for (int64_t e = w.n_succ; e < E; ++e) S.n_loop_closures += closure_ok(w.res[(size_t)e]) ? 1 : 0;
    for (int64_t v = 0; v < 3 * V; ++v) poses_out[v] = (double)est[v];
    if ((rc = dpg_gn_set_poses(c, poses_out))) return rc;
    if ((rc = gn_loop(c, P, poses_out, w.t2, now_ms(), &S.gn))) return rc;
    const double t3 = now_ms();
    S.n_factors = (int64_t)w.F.size();
    S.ms_icp = w.t2 - w.t1;
    S.ms_gn = t3 - w.t2;
    if (st) *st = S;
    return DPG_OK;
}

int dpg_reoptimize_inc(dpg_inc* g, int64_t V, const int32_t* pass, const float* est, const float* odom,
                       const dpg_icp_params* ip, const dpg_reopt_params* rp, double* poses_out, dpg_reopt_stats* st) {
    if (!g || V <= 0 || !pass || !est || !odom || !poses_out) return fail(DPG_ERR_ARG, "dpg_reoptimize_inc: bad arguments");
    Sweep w;
    int rc = reopt_sweep(dpg_inc_ctx(g), V, pass, est, odom, ip, rp, w);
    if (rc) return rc;
    dpg_reopt_stats& S = w.S;
    // addObservationConstraint per aligned pair (dpg_slam.cc:85-104); the slots of dropped closures go away
    w.F.resize((size_t)w.first_icp);
    if ((rc = append_icp_factors("dpg_reoptimize_inc", w.res.data(), w.edges, w.n_succ, w.I, w.F, S.n_loop_closures)))
        return rc;
    // the new ISAM2 + graph_ and its one update from the current estimates (dpg_slam.cc:36-39,111-119)
    std::vector<double> X0((size_t)(3 * V));
    for (int64_t v = 0; v < 3 * V; ++v) X0[(size_t)v] = (double)est[v];
    if ((rc = dpg_inc_reset(g))) return rc;
    dpg_inc_stats is;
    if ((rc = dpg_inc_update(g, V, X0.data(), w.F.data(), (int64_t)w.F.size(), &is))) return rc;
    if ((rc = dpg_inc_get_poses(g, poses_out, V))) return rc;
    const double t3 = now_ms();
    S.n_factors = (int64_t)w.F.size();
    S.ms_icp = w.t2 - w.t1;
    S.ms_gn = t3 - w.t2;
    S.gn.iterations = is.gn_iterations;
    S.gn.final_error = is.error;
    if (st) *st = S;
    return DPG_OK;
}

int dpg_add_node_pairs(dpg_inc* g, const float* cloud, int64_t n_pts, const float init_pose[3], const dpg_factor* extra,
                       int64_t n_extra, const int32_t* pairs, int64_t n_pairs, int32_t successive,
                       const dpg_icp_params* ip, dpg_add_node_stats* st) {
    if (!g || (!cloud && n_pts > 0) || n_pts < 0 || !init_pose || (n_extra > 0 && !extra) || n_extra < 0 ||
        n_pairs < 0 || (n_pairs > 0 && !pairs))
        return fail(DPG_ERR_ARG, "dpg_add_node_pairs: bad arguments");
    dpg_ctx* c = dpg_inc_ctx(g);
    const dpg_icp_params I = or_default(ip, dpg_icp_params_default);
    dpg_add_node_stats S;
    memset(&S, 0, sizeof(S));
    const int64_t V = dpg_inc_num_nodes(g);
    if (c->n_nodes != V) return fail(DPG_ERR_STATE, "scan store holds %lld nodes, graph %lld", (long long)c->n_nodes,
                                     (long long)V);
    for (int64_t e = 0; e < n_pairs; ++e)
        if (pairs[2 * e] < 0 || pairs[2 * e + 1] < 0 || pairs[2 * e] > V || pairs[2 * e + 1] > V || pairs[2 * e] == pairs[2 * e + 1])
            return fail(DPG_ERR_ARG, "dpg_add_node_pairs: pair %lld references a missing node", (long long)e);
    // createNode: the node's cloud joins the store (node id V).  Any failure after this point
    // takes the node out of the store again (and undoes a prepared update), so the store and the
    // graph keep the same node count and the next dpg_add_node can proceed.
    const int64_t offs[2] = {0, n_pts};
    const float dummy[2] = {0.f, 0.f};
    int rc = dpg_scans_append(c, n_pts > 0 ? cloud : dummy, offs, 1, I.downsample_icp_points_ratio);
    if (rc) return rc;
    struct Undo {
        dpg_ctx* c;
        dpg_inc* g;
        int64_t V;
        bool armed = true;
        ~Undo() {
            if (!armed) return;
            dpg_inc_abort_prepare(g);
            scans_truncate(c, V);
        }
    } undo{c, g, V};
    // estimates as float (dpg_nodes_ positions), the new node's initial pose last
    std::vector<double> est((size_t)(3 * std::max<int64_t>(V, 1)));
    if (V > 0 && (rc = dpg_inc_get_poses(g, est.data(), V))) return rc;
    std::vector<float> pf((size_t)(3 * (V + 1)));
    for (int64_t q = 0; q < 3 * V; ++q) pf[(size_t)q] = (float)est[(size_t)q];
    for (int k = 0; k < 3; ++k) pf[(size_t)(3 * V + k)] = init_pose[k];
    std::vector<int32_t> edges;
    if (successive && V >= 1) { edges.push_back((int32_t)(V - 1)); edges.push_back((int32_t)V); }
    edges.insert(edges.end(), pairs, pairs + 2 * n_pairs);
    const int64_t n_succ = (successive && V >= 1) ? 1 : 0;
    const int64_t E = (int64_t)edges.size() / 2;
    std::vector<dpg_factor> F(extra, extra + n_extra);
    if (E > 0) {
        const double t0 = now_ms();
        if ((rc = dpg_icp_batch_prepare(c, edges.data(), E, pf.data(), &I))) return rc;
        // nodes below V whose index is stale (a k-d tree / grid batch overwrote the buffers, or a
        // fresh upload was not indexed) are rebuilt with the new node
        if ((rc = icp_batch_run_from(c, std::min(V, c->idx_valid)))) return rc;
        // while the GPU aligns: the update's structure on the host, with every pair a factor may
        // come from (a loop closure that does not converge stays an explicit zero block)
        {
            std::vector<int32_t> pr(edges);
            for (int64_t k = 0; k < n_extra; ++k)
                if (extra[k].kind == DPG_FACTOR_BETWEEN) { pr.push_back(extra[k].i); pr.push_back(extra[k].j); }
            if ((rc = dpg_inc_prepare(g, 1, pr.data(), (int64_t)pr.size() / 2))) return rc;
        }
        std::vector<dpg_icp_result> res((size_t)E);
        if ((rc = batch_fetch(c, res.data(), nullptr, false))) return rc;
        S.ms_icp = now_ms() - t0;
        S.n_icp_edges = E;
        // successive: always (dpg_slam.cc:263-267); loop closures when converged (:295-301)
        if ((rc = append_icp_factors("dpg_add_node_pairs", res.data(), edges, n_succ, I, F, S.n_loop_closures))) return rc;
    } else if (c->icp_variant == DPG_ICP_ANGULAR && n_pts > 0) {   // no alignment: only the new node's index
        rc = dpg_launch_angle_index(c->ds.p, c->ds_off_dev.p + V, 1, c->max_ds, c->tree_pts.p, c->tree_idx.p,
                                    c->buckets.p + V * (int64_t)(dpg_angle_buckets() + 1), c->kernel_variant == 2,
                                    c->stream);
        if (rc) return fail(rc, "angle index build failed");
        if (c->idx_valid == V) c->idx_valid = V + 1;
    }
    const double init[3] = {(double)init_pose[0], (double)init_pose[1], (double)init_pose[2]};
    if ((rc = dpg_inc_update(g, 1, init, F.data(), (int64_t)F.size(), &S.update))) return rc;   // rolled back itself
    undo.armed = false;
    if (st) *st = S;
    return DPG_OK;
}

int dpg_add_node(dpg_inc* g, const float* cloud, int64_t n_pts, const int32_t* pass, const float init_pose[3],
                 const dpg_factor* extra, int64_t n_extra, const dpg_icp_params* ip, const dpg_reopt_params* rp,
                 int32_t non_successive, dpg_add_node_stats* st) {
    if (!g || !pass || !init_pose) return fail(DPG_ERR_ARG, "dpg_add_node: bad arguments");
    const dpg_reopt_params R = or_default(rp, dpg_reopt_params_default);
    const int64_t V = dpg_inc_num_nodes(g);
    // updatePoseGraphObsConstraints (dpg_slam.cc:273-304): loop-closure candidates (i, prev), i < V - 2,
    // by the float distance of the estimates (dpg_nodes_ positions are float), ascending i
    std::vector<int32_t> lc;
    if (non_successive && V > 1) {
        std::vector<double> est((size_t)(3 * V));
        int rc = dpg_inc_get_poses(g, est.data(), V);
        if (rc) return rc;
        const int64_t pv = V - 1;
        const float px = (float)est[(size_t)(3 * pv)], py = (float)est[(size_t)(3 * pv + 1)];
        for (int64_t i = 0; i < V - 2; ++i) {
            const float dx = (float)est[(size_t)(3 * i)] - px, dy = (float)est[(size_t)(3 * i + 1)] - py;
            const float dist = sqrtf(dx * dx + dy * dy);   // Eigen Vector2f::norm
            const float thr = pass[i] == pass[pv] ? R.max_node_dist_within_pass : R.max_node_dist_across_passes;
            if (dist <= thr) { lc.push_back((int32_t)i); lc.push_back((int32_t)pv); }
        }
    }
    return dpg_add_node_pairs(g, cloud, n_pts, init_pose, extra, n_extra, lc.data(), (int64_t)lc.size() / 2, 1, ip, st);
}

}  // extern "C"
