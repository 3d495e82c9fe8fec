/*
 * dpg_slam_c.h -- C ABI of the MI355X-native DPG-SLAM hot path.
 *
 * This library replaces the numerically hot part of BharathMasetty/DPG-SLAM:
 *   - DpgSLAM::runIcp            (src/dpg_slam/dpg_slam.cc:362-446, decl dpg_slam.h:630)
 *     which wraps pcl::IterativeClosestPoint<PointXYZ,PointXYZ>::align (dpg_slam.cc:387-416)
 *     and calculate_ICP_COV (src/icp_cov/cov_func_point_to_point.h:24, see dpg_icp_cov.h);
 *   - DpgSLAM::optimizeGraph     (src/dpg_slam/dpg_slam.cc:316-329, decl dpg_slam.h:464)
 *     which runs GTSAM ISAM2 / Gauss-Newton over PriorFactor<Pose2> / BetweenFactor<Pose2>
 *     built at dpg_slam.cc:44-75,178-183,227-238,331-338.
 *
 * All entry points are extern "C", take plain pointers + sizes, and return an int status
 * (0 = OK, negative = error; dpg_last_error() gives the message).  Buffers are caller-owned
 * HOST memory unless the parameter name ends in _dev (device memory on the context's GPU).
 * A context is thread-compatible (one per thread), not thread-safe -- the reference calls
 * all of these from the single ros::spin thread (dpg_slam_main.cc:328).
 */
#ifndef DPG_SLAM_C_H
#define DPG_SLAM_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPG_OK 0
#define DPG_ERR_ARG (-1)
#define DPG_ERR_HIP (-2)
#define DPG_ERR_STATE (-3)
#define DPG_ERR_SIZE (-4)
#define DPG_ERR_NUMERIC (-5)
#define DPG_ERR_INTERNAL (-6) /* a kernel failed its own consistency check (DPG_ICP_INTERNAL) */

/* Fixed reduction geometry of the ICP rigid fit (part of the algorithm's definition so that
 * CPU oracle and GPU agree bit for bit): lane l accumulates source points l, l+512, ... in
 * increasing order (fp64); each 64-lane wave folds acc[k] += acc[k + off], off = 32 ... 1, and
 * the eight wave totals combine as ((W0 + W1) + (W2 + W3)) + ((W4 + W5) + (W6 + W7)). */
#define DPG_ICP_LANES 512

/* ICP parameters: field names follow PoseGraphParameters (src/dpg_slam/parameters.h:105-141,
 * defaults :146,159,173,191,201,374,385,396,402) plus the PCL defaults the reference inherits
 * (Registration::min_number_correspondences_ = 3, DefaultConvergenceCriteria mse abs 1e-12). */
typedef struct dpg_icp_params {
    int32_t icp_maximum_iterations;              /* 500 */
    int32_t icp_use_reciprocal_correspondences;  /* 1 */
    double icp_maximum_transformation_epsilon;   /* 5e-9 */
    double icp_max_correspondence_distance;      /* 0.6 */
    int32_t ransac_iterations;                   /* 50 -- inert, as in PCL ICP */
    int32_t downsample_icp_points_ratio;         /* 5 */
    float laser_x_variance;                      /* 0.5 */
    float laser_y_variance;                      /* 0.5 */
    float laser_theta_variance;                  /* 0.3 */
    int32_t min_number_correspondences;          /* 3 (pcl::Registration default) */
    double mse_threshold_absolute;               /* 1e-12 (pcl DefaultConvergenceCriteria) */
} dpg_icp_params;

/* Per-edge ICP outcome (runIcp's out-param + return value, dpg_slam.cc:433-445). */
typedef struct dpg_icp_result {
    float T[6];          /* final transformation, rows: T00 T01 T03 / T10 T11 T13 (z row = e3) */
    float z[3];          /* measurement (T03, T13, atan2(T10, T00)) -- dpg_slam.cc:434-439 */
    int32_t converged;   /* icp.hasConverged() (max iterations counts as converged, as in PCL) */
    int32_t iterations;  /* nr_iterations_ */
    int32_t n_corr;      /* correspondences of the last iteration */
    int32_t status;      /* DPG_ICP_* below */
    int32_t pad;
    double fitness;      /* MSE of the last iteration's correspondences */
} dpg_icp_result;

#define DPG_ICP_OK 0
#define DPG_ICP_TOO_FEW_CORR 1   /* fewer than min_number_correspondences -> converged = 0 */
#define DPG_ICP_NON_PLANAR 2     /* est_transform(2,2) != 1 (dpg_slam.cc:422-426); never produced by
                                    the planar closed form, kept for ABI parity */
#define DPG_ICP_INTERNAL 3       /* kernel self-check failed (a bug: never expected) */

/* Factors (R9/R10).  info = diagonal information (1/sigma^2 for noiseModel::Diagonal::Sigmas,
 * 1/variance for noiseModel::Gaussian::Covariance of a diagonal matrix, dpg_slam.cc:335). */
#define DPG_FACTOR_PRIOR 0
#define DPG_FACTOR_BETWEEN 1
typedef struct dpg_factor {
    int32_t kind;      /* DPG_FACTOR_PRIOR | DPG_FACTOR_BETWEEN */
    int32_t i;         /* first key (prior: the key) */
    int32_t j;         /* second key (between) */
    int32_t pad;
    double z[3];       /* measured Pose2 (x, y, theta): prior mean or between measurement */
    double info[3];    /* diagonal information */
} dpg_factor;          /* 64 bytes */

typedef struct dpg_gn_params {
    int32_t max_iterations;      /* 100 (GaussNewtonParams.maxIterations, dpg_slam_main.cc:262) */
    int32_t use_error_criteria;  /* 1: GTSAM checkConvergence on the error; 0: stop on max|delta| */
    double delta_tol;            /* 1e-10: batch-GN target */
    double relative_error_tol;   /* 1e-5 (GaussNewtonParams.relativeErrorTol) */
    double absolute_error_tol;   /* 1e-5 (NonlinearOptimizerParams default) */
    double pcg_rel_tol;          /* 1e-12: PCG stops when |r| <= tol * |b| */
    int32_t pcg_max_iterations;  /* 20000 */
    int32_t pcg_check_every;     /* PCG iterations between host convergence checks (GPU only) */
    int32_t linear_solver;       /* DPG_SOLVER_CHOLESKY (default, GTSAM's CHOLESKY) | DPG_SOLVER_PCG */
    int32_t reuse_factorization; /* 1 (default): once the last step's max|delta| < refactor_delta, solve
                                    with the previous Cholesky factor (a chord step: same fixed point
                                    g(X) = 0, H barely changes that close to it); 0: refactor every
                                    iteration (plain Gauss-Newton) */
    double refactor_delta;       /* 1e-3 (tools/refactor_sweep.sh: config 4 converges in 8 iterations
                                    with 3 factorizations instead of 7 with 4, 2.4 % less per step) */
} dpg_gn_params;

#define DPG_SOLVER_CHOLESKY 0    /* supernodal multifrontal Cholesky on the GPU */
#define DPG_SOLVER_PCG 1         /* block-Jacobi preconditioned CG on the GPU */

typedef struct dpg_gn_stats {
    int32_t iterations;
    int32_t pcg_iterations;      /* total over all GN iterations */
    double initial_error;        /* 0.5 * sum ||e||^2_info at the initial values */
    double final_error;
    double last_delta_inf;
    double ms_total;
    double ms_per_iteration;
} dpg_gn_stats;

typedef struct dpg_ctx dpg_ctx;

/* ---- library / context ---- */
const char* dpg_last_error(void);
const char* dpg_version(void);
void dpg_icp_params_default(dpg_icp_params* p);
void dpg_gn_params_default(dpg_gn_params* p);
/* device = HIP device ordinal; returns NULL (and sets dpg_last_error) when no GPU is usable. */
dpg_ctx* dpg_ctx_create(int device);
/* Also destroys every incremental graph (dpg_inc_create / dpg_inc_load) and DPG store
 * (dpg_dpg_create) still alive on ctx; their handles are invalid afterwards. */
void dpg_ctx_destroy(dpg_ctx* ctx);
/* Multi-GPU context (SURVEY 8b "dpg_ctx_create(int n_gpus)", 8e): ONE host process drives n_gpus
 * devices (devices[k], or 0 .. n_gpus-1 when devices is NULL), one stream per device and one RCCL
 * communicator per device (ncclCommInitAll over xGMI).  The same entry points then run sharded,
 * so a single-threaded host -- the reference's ROS node (dpg_slam_main.cc:284-331) -- uses N GPUs
 * through the unchanged call sites:
 *   dpg_scans_upload / dpg_scans_append   every device holds every scan;
 *   dpg_icp_batch_prepare / _run / _fetch edge e is aligned on device e mod n_gpus, all devices
 *                                         concurrently; results (and covariance blocks) come back
 *                                         in the caller's order; _kernel_ms is the slowest device
 *                                         (dpg_ctx_set_icp_schedule: once every edge's cost is
 *                                         known from an earlier run, a longest-processing-time
 *                                         assignment instead);
 *   dpg_optimize_graph, dpg_reoptimize,   every device holds the factor list and linearizes its
 *   dpg_gn_setup + _take_icp_measurements share (factor f mod n, and each ICP slot on the device
 *   + _set_poses + dpg_gn_run             that aligned its edge); per Gauss-Newton iteration ONE
 *                                         ncclAllReduce(sum, fp64) of the packed [H upper | g |
 *                                         chi2]; every device factors and solves the identical
 *                                         system and takes its own (identical) stop / chord
 *                                         decisions on the device (poses bitwise equal on all
 *                                         devices; the loop checks their reports agree).
 * dpg_run_icp, icp_cov_calculate / icp_cov_sandwich, dpg_get_map and dpg_loop_closure_candidates
 * run on the first device.  The per-iteration step API (dpg_gn_assemble / _solve_retract* /
 * _fetch), the trace and the incremental graph (dpg_inc_create: per-node updates are
 * latency-bound, one GPU) need a single-device context.  n_gpus = 1 gives a context whose calls
 * take the sharded paths with one rank (RCCL included): its results equal dpg_ctx_create's byte
 * for byte. */
dpg_ctx* dpg_ctx_create_multi(int32_t n_gpus, const int32_t* devices);
/* One process per GPU (torchrun and the like): this process's `device` is global rank `rank` of
 * `world`; the RCCL communicator is built from the id rank 0 made with dpg_nccl_unique_id and the
 * caller handed to every rank (ncclCommInitRank).  The batched calls above then act on the whole
 * job: dpg_icp_batch_prepare takes ALL edges and aligns this rank's share, dpg_icp_batch_fetch
 * returns every edge's result (a collective: every rank calls it), the Gauss-Newton calls
 * all-reduce across ranks.  Every rank must make the same calls with the same arguments. */
#define DPG_NCCL_ID_BYTES 128
int dpg_nccl_unique_id(void* id_out /*[DPG_NCCL_ID_BYTES]*/);
dpg_ctx* dpg_ctx_create_rank(int32_t device, const void* nccl_id, int32_t rank, int32_t world);
/* The same one-process-per-GPU form over the CALLER's collectives instead of RCCL: a host that
 * already runs a communicator (MPI, gloo), or ranks that share one card (RCCL refuses a second rank
 * on a device -- the one-GPU test box runs the world > 1 rank form this way).  Three blocking calls
 * on host memory, made by every rank in the same order with the same sizes, each returning 0 on
 * success: the float sum of the alignment costs (the LPT plan), the all-gather of the results, the
 * fp64 sum of the packed [H upper | g | chi2 | votes] per Gauss-Newton iteration. */
typedef struct dpg_coll_ops {
    void* user;
    int (*allreduce_sum_f64)(void* user, double* buf, int64_t n);               /* in place */
    int (*allreduce_sum_f32)(void* user, float* buf, int64_t n);                /* in place */
    int (*allgather)(void* user, const void* send, void* recv, int64_t bytes);  /* recv: world * bytes, rank order */
} dpg_coll_ops;
dpg_ctx* dpg_ctx_create_rank_ops(int32_t device, const dpg_coll_ops* ops, int32_t rank, int32_t world);
/* Host helpers of the multi-device forms (no device call): the batch's assignment over `world` ranks
 * -- cost == NULL: edge e on rank e mod world in the caller's order; else longest-processing-time
 * (longest first to the least-loaded rank; ties: lower index, lower rank) -- as owner[e] and every
 * rank's dispatch order (rank 0's counts[0] edges first, then rank 1's, ...); and the rank form's
 * all-gathered results (slice r = rank r's records, its edges ascending, `slice` records reserved
 * per rank) back into the caller's order. */
int dpg_shard_plan(const float* cost, int64_t n_edges, int32_t world, int32_t* owner, int64_t* dispatch,
                   int64_t* counts);
int dpg_shard_reassemble(const int32_t* owner, int64_t n_edges, int32_t world, int64_t slice, int64_t rec_bytes,
                         const void* gathered, void* out);
/* Test / rehearsal form: k "devices" that are k contexts on ONE device sharing one stream, the
 * all-reduce a device-side sum in rank order.  Every sharded path of the multi-device forms runs
 * with k > 1 on one card (k <= 16). */
dpg_ctx* dpg_ctx_create_virtual(int32_t k, int32_t device);
int32_t dpg_ctx_num_gpus(dpg_ctx* ctx);   /* local devices: 1 for dpg_ctx_create and the rank form */
int32_t dpg_ctx_num_ranks(dpg_ctx* ctx);  /* ranks of the collective (ncclCommCount; k virtual; 1) */
int32_t dpg_ctx_rank(dpg_ctx* ctx);       /* global rank of the first local device */
/* Batched ICP dispatch (results are identical for both): DPG_ICP_SCHEDULE_CALLER -- edge e on rank
 * e mod ranks, in the caller's order; DPG_ICP_SCHEDULE_MEASURED (default) -- the same until every
 * edge of the staged batch has a measured cost (iterations x points, from an earlier run of the
 * same (target, source) pair: a batch run again, or the next sweep), then a longest-processing-time
 * assignment over the ranks and longest-first dispatch on each, so that the alignments that bound
 * a launch start first. */
#define DPG_ICP_SCHEDULE_CALLER 0
#define DPG_ICP_SCHEDULE_MEASURED 1
int dpg_ctx_set_icp_schedule(dpg_ctx* ctx, int32_t schedule);
/* Options of the supernodal Cholesky (per context; every device of a multi-device context), taken
 * by the next graph set up on it (dpg_gn_setup, dpg_optimize_graph, dpg_reoptimize, dpg_inc_create).
 * The defaults are the measured choices; the others are cross-checks and A/B
 * references that must give the same solution to rounding. */
#define DPG_ORDER_AUTO 0   /* nested dissection: the shorter critical path of two separator rules */
#define DPG_ORDER_MD 1     /* minimum degree */
#define DPG_ORDER_ND 2     /* nested dissection, round 2's separator rule alone */
typedef struct dpg_solver_options {
    int32_t order;               /* DPG_ORDER_AUTO */
    int32_t fused;               /* 1: one-launch DAG factorization + solves when every front fits LDS;
                                    0: the level-scheduled factorization */
    int32_t solve_stage;         /* doubles of L staged in LDS by the DAG solves; -1: what fills 80 KB */
    int32_t solve_maxseg;        /* ancestor row segments per front in the backward solve; -1: all */
    int32_t solve_dinv;          /* 1: the solves use inverted diagonal blocks (0: substitution chains) */
    int32_t merge_single;        /* 1: supernodes merge only along single-child chains (round 1's rule) */
    int32_t max_supernode_cols;  /* 64 block columns */
    int32_t solve_inv_cols;      /* 0 (never): fronts with at least this many pivot columns get their
                                    diagonal block's inverse L11^-1 after each factorization (beside
                                    the backward solve in the pipelined loop), and the chord steps'
                                    triangular solves apply it as one product instead of a
                                    substitution chain -- 14 us off each solve, but the inversion and
                                    its stream hand-offs cost more */
    double relax_fraction;       /* 0.3: explicit-zero budget of relaxed supernodes */
} dpg_solver_options;
void dpg_solver_options_default(dpg_solver_options* o);
int dpg_ctx_set_solver_options(dpg_ctx* ctx, const dpg_solver_options* o);
/* Run all work of this context on an external hipStream_t (e.g. torch's current stream); on a
 * multi-GPU context it applies to the first device only. */
int dpg_ctx_set_stream(dpg_ctx* ctx, void* hip_stream);
int dpg_ctx_synchronize(dpg_ctx* ctx);

/* ---- host-side data path helpers (R1-R3, no GPU) ---- */
/* MeasurementPoint + createNode + getCachedPointCloudFromNode (dpg_measurement.h:41-46,102-104,
 * dpg_slam.cc:488-513, dpg_node.cc:8-25): polar scan -> base_link cloud, MAX_RANGE dropped.
 * Returns the number of points written to xy_out (capacity n_ranges points). */
int64_t dpg_scan_to_cloud(const float* ranges, int64_t n_ranges, float angle_min, float angle_max,
                          float range_max, float laser_x, float laser_y, float laser_theta,
                          float* xy_out);
/* R1 over a scan set: ranges[V][n_beams] -> concatenated clouds, offsets_out[V+1] (capacity
 * V * n_beams points).  Returns the total number of points. */
int64_t dpg_scans_to_clouds(const float* ranges, int64_t n_nodes, int64_t n_beams, float angle_min,
                            float angle_max, float range_max, float laser_x, float laser_y,
                            float laser_theta, float* xy_out, int64_t* offsets_out);
/* downsamplePointCloud (dpg_slam.cc:346-360). Returns the number of points written. */
int64_t dpg_downsample_cloud(const float* xy, int64_t n, int32_t ratio, float* xy_out);
/* math_utils::inverseTransformPoint (math_utils.cc:21-35): pose of a in b's frame. */
void dpg_inverse_transform_point(const float a[3], const float b[3], float out[3]);
/* math_utils::transformPoint (math_utils.cc:6-19). */
void dpg_transform_point(const float p[3], const float frame[3], float out[3]);
/* runIcp guess (dpg_slam.cc:364-378): 2x3 float matrix rows (c,-s,tx / s,c,ty). */
void dpg_icp_guess(const float pose_src[3], const float pose_tgt[3], float guess_out[6]);
/* R9 factor builders: odometry BetweenFactor with the motion-model sigmas (dpg_slam.cc:53-75),
 * ICP BetweenFactor with the calculate_ICP_COV diagonal (dpg_slam.cc:331-338). */
int dpg_odometry_factor(const float odom_prev[3], const float odom_cur[3], int32_t i_prev, int32_t i_cur,
                        float transl_from_transl, float transl_from_rot, float rot_from_transl,
                        float rot_from_rot, dpg_factor* out);
void dpg_icp_factor(const dpg_icp_result* r, int32_t from_node, int32_t to_node,
                    const dpg_icp_params* p, dpg_factor* out);
/* dpg_odometry_factor over n pairs: factor k between odometry poses odom[i_prev[k]] and
 * odom[i_cur[k]] (odom: [n_odom][3]), into out[k] -- the reference's per-node loop of reoptimize
 * (dpg_slam.cc:53-75) in one call; returns the first error (out[k] of a failed pair unset). */
int dpg_odometry_factors(const float* odom, int64_t n_odom, const int32_t* i_prev, const int32_t* i_cur, int64_t n,
                         float transl_from_transl, float transl_from_rot, float rot_from_transl, float rot_from_rot,
                         dpg_factor* out);

/* ---- synthetic workload generator (seeded, deterministic) ---- */
/* World: axis-aligned rooms + random boxes in [0, world_size]^2; segments [n][4] (x0,y0,x1,y1). */
int64_t dpg_synth_world(uint64_t seed, float world_size, float* segs_out, int64_t max_segs);
/* Ground-truth trajectory: 1 m steps with heading noise, collision-free w.r.t. the world. */
int dpg_synth_trajectory(uint64_t seed, int64_t n_nodes, const float* segs, int64_t n_segs,
                         float world_size, float step, double* gt_out /*[n][3]*/);
/* Ray-cast laser scans (laser pose in base_link), Gaussian range noise, >= range_max kept as
 * range_max (MAX_RANGE).  ranges_out[n_nodes][n_beams]. */
int dpg_synth_scans(const double* gt, int64_t n_nodes, const float* segs, int64_t n_segs,
                    int32_t n_beams, float angle_min, float angle_max, float range_max,
                    float laser_x, float laser_y, float laser_theta, float noise_sigma,
                    uint64_t seed, int32_t n_threads, float* ranges_out);

/* ---- ICP (runIcp) ---- */
/* One alignment, mirroring DpgSLAM::runIcp(node_1 = target, node_2 = source, ...).
 * src_xy / tgt_xy are the FULL base_link clouds of node_2 / node_1 (the ICP downsamples them
 * by params->downsample_icp_points_ratio; the covariance uses the full clouds, dpg_slam.cc:430).
 * pose_src / pose_tgt: estimated poses (x, y, theta) of node_2 / node_1.
 * cov_out (3x3 row-major) receives ICP_COV; hess_out (nullable) the diagnostic [x,y,yaw] block.
 * Returns DPG_OK; the boolean runIcp result is result->converged && status == DPG_ICP_OK. */
int dpg_run_icp(dpg_ctx* ctx, const float* src_xy, int64_t n_src, const float* tgt_xy, int64_t n_tgt,
                const float pose_src[3], const float pose_tgt[3], const dpg_icp_params* params,
                dpg_icp_result* result, double cov_out[9], double hess_out[9]);

/* Batched, device-resident form (the GPU entry point).
 * 1) upload all node clouds once: pts_xy = concatenated full clouds, node_offsets[V+1]. */
int dpg_scans_upload(dpg_ctx* ctx, const float* pts_xy, const int64_t* node_offsets, int64_t n_nodes,
                     int32_t downsample_ratio);
/* 2) stage an edge batch: edges[e] = {node_1 (target), node_2 (source)}, poses[V][3] float. */
int dpg_icp_batch_prepare(dpg_ctx* ctx, const int32_t* edges, int64_t n_edges, const float* poses,
                          const dpg_icp_params* params);
/* 3) run ICP (+ covariance block when compute_cov) over the staged edges, asynchronously on the
 * context stream.  trace_iters > 0 records the per-iteration correspondence indices of every
 * edge (test mode; see dpg_icp_batch_fetch_trace). */
int dpg_icp_batch_run(dpg_ctx* ctx, int32_t compute_cov, int32_t trace_iters);
/* 4) copy results back (any pointer may be NULL).  cap: the number of records results (and
 * hess, [cap][9]) can hold; DPG_ERR_SIZE, with nothing written, when the staged batch is larger
 * (dpg_icp_batch_size tells how many are staged -- a sweep or dpg_add_node may have staged more
 * than the caller's own edges). */
int dpg_icp_batch_fetch(dpg_ctx* ctx, dpg_icp_result* results, double* hess /*[cap][9]*/, int64_t cap);
/* Edges of the staged batch -- dpg_icp_batch_prepare's, or the batch a sweep (dpg_reoptimize) or
 * dpg_add_node staged last: the number of records dpg_icp_batch_fetch writes. */
int64_t dpg_icp_batch_size(dpg_ctx* ctx);
/* trace_cap: int32 elements trace can hold; DPG_ERR_SIZE when E * trace_iters * max_src exceeds it
 * (call with trace = NULL first to learn max_src). */
int dpg_icp_batch_fetch_trace(dpg_ctx* ctx, int32_t* trace /*[E][trace_iters][max_src]*/, int64_t trace_cap,
                              int64_t* max_src_out);
/* Device time of the last ICP / covariance kernels (ms, HIP events on the context stream). */
float dpg_icp_batch_kernel_ms(dpg_ctx* ctx);
float dpg_cov_batch_kernel_ms(dpg_ctx* ctx);
/* 1: the last batch's covariance kernel ran on the context's second stream, beside what followed
 * the ICP on its stream (the pose graph does not read it; DPG_COV_OVERLAP=0 keeps stream order) */
int32_t dpg_cov_batch_overlapped(dpg_ctx* ctx);
/* Device time of the per-node index build (k-d trees / angle index) that precedes the ICP kernel. */
float dpg_kdtree_build_ms(dpg_ctx* ctx);
/* Nearest-neighbour machinery of the ICP kernel; all give bit-identical results. */
#define DPG_ICP_ANGULAR 3  /* per-node angle-sorted clouds + buckets, windowed scans (default) */
#define DPG_ICP_KDTREE 2   /* per-node k-d trees, seeded search, static-frame reciprocal test */
#define DPG_ICP_GRID 1     /* uniform LDS grid, all-pairs reverse keys by LDS atomics */
int dpg_ctx_set_icp_variant(dpg_ctx* ctx, int32_t variant);
/* Angular variant tuning (results are identical for every value): a point whose search window
 * holds more than `cap` candidates is handed to the workgroup's cooperative queue, where a whole
 * wave scans it; 0 scans every window in its own lane.  Default 256.  Tested values: 0, 1 (nearly
 * every window queued, so the 64-item queue overflows in every iteration and the rest is scanned
 * in-lane), 8 and 256, each byte-equal to the oracle on near-origin, collinear, tied and
 * unequal-size clouds and one cloud size per kernel form (tests/test_icp_adversarial.py). */
int dpg_ctx_set_icp_defer_cap(dpg_ctx* ctx, int32_t cap);
/* The batched covariance that runs beside the pose graph (dpg_icp_batch_run with covariance, its own
 * stream): at most n workgroups, each taking edges in turn, so the pose graph's kernels find free
 * compute units while it runs; 0 = one workgroup per edge.  Default 256 -- one per compute unit
 * (config 4, one process A/B: 8.567 ms per step at 0, 8.524 at 256, 8.742 at 512; fewer than 64
 * stretch it past the pose graph).  Results are identical for every n. */
int dpg_ctx_set_cov_workgroups(dpg_ctx* ctx, int32_t n);
/* Diagnostic: the angular ICP kernel's form (0 = the default; others are A/B references that must give
 * byte-identical results, tools/icp_var_ab.py): 1 = the kernel's previous form (variant 4), 2 = the
 * default kernel after the angle index built by its previous bitonic network. */
int dpg_ctx_set_icp_kernel_variant(dpg_ctx* ctx, int32_t variant);
/* Sum over edges of iterations x (8N + 8M + 8N) -- algorithmic bytes of the correspondence
 * search for the last run, computed on device and copied back. */
double dpg_icp_batch_algorithmic_bytes(dpg_ctx* ctx);

/* ---- pose-graph Gauss-Newton (optimizeGraph) ---- */
/* Single call, batch GN to convergence.  poses_inout[V][3] double. */
int dpg_optimize_graph(dpg_ctx* ctx, double* poses_inout, int64_t n_nodes, const dpg_factor* factors,
                       int64_t n_factors, const dpg_gn_params* params, dpg_gn_stats* stats);

/* Step API for the edge-sharded multi-GPU solve (one RCCL all-reduce of the packed [H|b|chi2]
 * buffer per iteration, done by the caller between assemble and solve).
 * factors: ALL factors of the graph (the sparsity pattern is global); this rank assembles only
 * factors[shard_begin, shard_end). */
int dpg_gn_setup(dpg_ctx* ctx, int64_t n_nodes, const dpg_factor* factors, int64_t n_factors,
                 int64_t shard_begin, int64_t shard_end, const dpg_gn_params* params);
/* Overwrite the measurement/information of factors [first, first+count) with the ICP batch
 * results of edges [0, count) of the last dpg_icp_batch_run (device to device; multi-device forms:
 * count = the whole batch, each slot on the device that aligned it).  Edges
 * [0, n_always) always become factors (successive scans, dpg_slam.cc:85-89); the others only when
 * the alignment converged (loop closures, dpg_slam.cc:101-104) -- a dropped edge keeps its slot
 * with zero information, which adds nothing to H, g or the error. */
int dpg_gn_take_icp_measurements(dpg_ctx* ctx, int64_t first_factor, int64_t count, int64_t n_always,
                                 const dpg_icp_params* params);
int64_t dpg_gn_hb_size(dpg_ctx* ctx);   /* doubles in the packed buffer */
/* Host clock (ms) of the last dpg_gn_setup's parts, in this order: the pattern, contribution lists
 * and BSR rows; the Cholesky's symbolic analysis (ordering, supernodes); its plan (these three
 * before the setup waits for the context's stream; the lists and rows are built beside the other
 * two once the pairs are known); the wait + device allocations + uploads; the Cholesky's upload. */
int dpg_gn_setup_profile(dpg_ctx* ctx, double out[5]);
int dpg_gn_set_poses(dpg_ctx* ctx, const double* poses);
int dpg_gn_get_poses(dpg_ctx* ctx, double* poses);
/* Linearize the local shard at the current poses into hb_dev (overwritten, not accumulated). */
int dpg_gn_assemble(dpg_ctx* ctx, double* hb_dev);
/* Solve (sum of all shards in hb_dev) and retract.  Blocking: returns max|delta| and the error
 * 0.5*chi2 at the linearization point. */
int dpg_gn_solve_retract(dpg_ctx* ctx, const double* hb_dev, double* delta_inf, double* error,
                         int32_t* pcg_iterations);
/* The same, enqueued only (no host synchronisation with the Cholesky solver): the GN loop then
 * re-linearizes (dpg_gn_assemble, [all-reduce]) and reads everything it decides on with ONE
 * dpg_gn_fetch: out = {max|delta| of the last retraction, error of hb_dev, solver status
 * (0 = ok, 1 = H not positive definite, 2 = solver timeout)}. */
int dpg_gn_solve_retract_async(dpg_ctx* ctx, const double* hb_dev);
int dpg_gn_fetch(dpg_ctx* ctx, const double* hb_dev, double out[3]);
/* The whole Gauss-Newton loop of the setup (its parameters) from the poses of the last
 * dpg_gn_set_poses, natively: assemble, then per iteration solve + retract + re-linearize with the
 * stop and chord decisions taken on the device (multi-device forms: sharded assembly and one
 * all-reduce per iteration); poses_out[V][3] (may be NULL) receives the result. */
int dpg_gn_run(dpg_ctx* ctx, double* poses_out, dpg_gn_stats* stats);
/* Cholesky factorizations since the last dpg_gn_set_poses (the other solves reused one). */
int32_t dpg_gn_factorizations(dpg_ctx* ctx);
float dpg_gn_last_assemble_ms(dpg_ctx* ctx);
float dpg_gn_last_solve_ms(dpg_ctx* ctx);

/* ---- marginal covariances (gtsam::Marginals, dpg_slam_main.cc:272-279) ----
 * The 3x3 diagonal blocks of Sigma = H^-1, H = sum A^T Omega A, and the off-diagonal blocks inside
 * the Cholesky factor's pattern, by one selected-inversion pass over the factor's fronts on the
 * device (a small multiple of one factorization) instead of three solves per node.
 * Tangent space: each block is in the pose's own frame (GTSAM's right perturbation):
 * rows and columns are (dx, dy, dtheta) along the pose's body axes.  With R the rotation by the
 * pose's theta, the map-frame xy covariance is R Sxy R^T.
 * Linearization point: the graph of the last dpg_gn_setup at its CURRENT poses -- those of
 * dpg_gn_set_poses or the result of dpg_gn_run.  The call re-linearizes there and factors (the loop
 * may hold an earlier iterate's factor after a chord step); it does not change the poses, the step
 * history or the factorization count, so dpg_gn_set_poses + dpg_gn_run give bitwise the same
 * result with or without a marginals call in between.
 * Errors (cov_out is not written on any of them): DPG_ERR_ARG -- a node out of range, a pair of
 * nodes that share no factor (only H's own blocks are offered, not what fill adds to L's pattern);
 * DPG_ERR_STATE -- no graph set up, a graph without a Cholesky (linear_solver = DPG_SOLVER_PCG), or
 * a context of more than one rank: the multi-device forms (dpg_ctx_create_multi / _virtual / _rank)
 * do not compute marginals; DPG_ERR_NUMERIC -- H is not positive definite. */
/* marginalCovariance(key): cov_out[n][9] row-major.  nodes == NULL: every node in order (n = V). */
int dpg_gn_marginals(dpg_ctx* ctx, const int32_t* nodes, int64_t n, double* cov_out /*[n][9]*/);
/* joint blocks Sigma(i, j) (rows i, columns j) for pairs that share a factor; Sigma(j, i) is its
 * transpose */
int dpg_gn_marginal_pairs(dpg_ctx* ctx, const int32_t* pairs /*[n][2]*/, int64_t n, double* cov_out /*[n][9]*/);
/* ---- joint marginals of any nodes (gtsam::Marginals::jointMarginalCovariance) ----
 * Blocks of Sigma for ANY nodes, sharing a factor or not: with P H P^T = L L^T,
 * Sigma(i, j) = (L^-1 E_i)^T (L^-1 E_j), E_q the three unit columns of node q.  L^-1 E_q is nonzero
 * only on the fronts between q's and the root of its elimination tree, so a query is one forward
 * substitution along one root path plus dot products over the part two paths share (DESIGN.md,
 * "Joint marginals").  Tangent frames, the linearization point, "does not change the poses, the
 * step history or the factorization count" and the DPG_ERR_STATE / DPG_ERR_NUMERIC cases are those
 * of dpg_gn_marginals; DPG_ERR_ARG -- a node out of range, a NULL list with n > 0, n < 0.  cov_out
 * is not written on any error.  All solver options are supported (solve_inv_cols keeps L11^-1 in a
 * buffer of its own: the fronts still hold L11).  dpg_gn_marginal_pairs is unchanged: it still
 * refuses pairs without a common factor. */
/* Sigma(i, j) (rows i, columns j) for any i, j in range -- i == j, repeated nodes and repeated
 * pairs included; the block of (j, i) is bitwise the transpose of the block of (i, j) */
int dpg_gn_cross_covariances(dpg_ctx* ctx, const int32_t* pairs /*[n][2]*/, int64_t n, double* cov_out /*[n][9]*/);
/* jointMarginalCovariance(nodes): the full covariance over `nodes` in the caller's order, exactly
 * symmetric (each block computed once and mirrored) */
int dpg_gn_joint_marginal(dpg_ctx* ctx, const int32_t* nodes, int64_t n, double* cov_out /*[3n][3n] row-major*/);
/* The 3x3 covariance of the relative pose z = X_i^-1 X_j in z's own tangent frame:
 * J [[Sii, Sij], [Sji, Sjj]] J^T, J = [A_i A_j] the Jacobians of the Between linearization at zero
 * error (A_j = I, A_i = -Ad(z^-1)), taken at the poses Sigma was computed at.  Exactly symmetric;
 * the zero matrix for i == j.  With the candidate's measured z_m, e = Local(z, z_m) and
 * e^T (cov + cov_m)^-1 e is the Mahalanobis gate of a loop-closure candidate. */
int dpg_gn_relative_covariances(dpg_ctx* ctx, const int32_t* pairs /*[n][2]*/, int64_t n, double* cov_out /*[n][9]*/);
/* Diagnostic (tools/joint_probe.py): one dpg_gn_cross_covariances with its kernels timed by HIP
 * events.  out = {path solve ms, dot ms, the longest root path of the analysis in fronts, in pivot
 * scalars}; cap >= 4. */
int dpg_gn_joint_profile(dpg_ctx* ctx, const int32_t* pairs /*[n][2]*/, int64_t n, double* out, int64_t cap);
/* one call: set up the graph (default parameters; it becomes the context's graph), linearize at
 * poses, factor, invert */
int dpg_marginal_covariances(dpg_ctx* ctx, const double* poses, int64_t n_nodes, const dpg_factor* factors,
                             int64_t n_factors, const int32_t* nodes, int64_t n, double* cov_out);
/* Diagnostic (tools/marginals_probe.py): dpg_gn_marginals of every node, timed by HIP events.
 * out = {assembly ms, factorization + solve ms, elimination-tree levels, bytes of the Sigma and
 * work buffers, then the ms of each selected-inversion launch, the roots' level first}; returns
 * the number of values written (negative: an error). */
int64_t dpg_gn_marginals_profile(dpg_ctx* ctx, double* out, int64_t cap);

/* ---- re-linearisation sweep (DpgSLAM::reoptimize, dpg_slam.cc:35-120) ---- */
typedef struct dpg_reopt_params {
    float max_node_dist_within_pass;    /* 5.0 (parameters.h:212) */
    float max_node_dist_across_passes;  /* 2.0 (parameters.h:224) */
    float new_pass_std_dev[3];          /* prior sigmas x, y, theta: 0.2, 0.2, 0.15 (parameters.h:264-274) */
    float motion_model[4];              /* transl<-transl, transl<-rot, rot<-transl, rot<-rot: 0.4 each
                                           (parameters.h:279-309) */
    int32_t odometry_constraints;       /* 1 (parameters.h:364) */
} dpg_reopt_params;

typedef struct dpg_reopt_stats {
    int64_t n_factors;          /* priors + odometry + ICP factor slots */
    int64_t n_icp_edges;        /* successive + loop-closure candidates (all aligned) */
    int64_t n_candidates;       /* loop-closure candidates (j, i), j < i - 1, within the distance rule */
    int64_t n_loop_closures;    /* candidates whose alignment converged (became factors) */
    double ms_candidates;       /* GPU candidate search incl. the copy back of the pair list */
    double ms_icp;              /* batched ICP (angle index + kernel) */
    double ms_gn;               /* graph setup (symbolic analysis) + Gauss-Newton */
    dpg_gn_stats gn;
} dpg_reopt_stats;

void dpg_reopt_params_default(dpg_reopt_params* p);

/* The candidate pairs of the sweep (dpg_slam.cc:91-98): for i ascending, j = 0 .. i-2 ascending,
 * (j, i) when the float distance of the estimated positions est_poses[j] - est_poses[i] (Eigen
 * Vector2f::norm) is <= max_node_dist_within_pass (same pass_numbers) or
 * <= max_node_dist_across_passes.  Computed on the GPU; writes min(count, cap) pairs {j, i} and
 * returns the count (negative: error). */
int64_t dpg_loop_closure_candidates(dpg_ctx* ctx, int64_t n_nodes, const int32_t* pass_numbers,
                                    const float* est_poses /*[V][3]*/, float max_dist_within_pass,
                                    float max_dist_across_passes, int32_t* pairs_out /*[cap][2]*/, int64_t cap);

/* The whole sweep on the uploaded scans (dpg_scans_upload of all V nodes):
 *   factors per node i in order: a prior (0, 0, 0) on the first node of each pass, otherwise the
 *   odometry Between (i-1, i) from odom_only (if odometry_constraints); the ICP edges: every
 *   successive pair (i-1, i) (always a factor, dpg_slam.cc:85-89) and every loop-closure
 *   candidate (j, i) (a factor when the alignment converged, dpg_slam.cc:101-104) -- one batched
 *   ICP of all of them from the estimated poses; then batch Gauss-Newton from est_poses (the
 *   ISAM2 update of optimizeGraph, run to convergence: SURVEY Q1/Q6).
 * poses_out[V][3] (double) receives the optimised poses. */
/* DpgSLAM::GetMap (dpg_slam.cc:555-575) over the uploaded full clouds: every node's base_link
 * points in the map frame (transformPoint with the node's estimated pose), one point in
 * display_points_fraction (10, parameters.h:22) by the running index over all nodes.  Writes
 * min(count, cap) points and returns the count, ceil(P / fraction) (negative: error). */
int64_t dpg_get_map(dpg_ctx* ctx, const float* est_poses /*[V][3]*/, int32_t display_points_fraction,
                    float* map_out /*[cap][2]*/, int64_t cap);
float dpg_get_map_kernel_ms(dpg_ctx* ctx);   /* device time of the last dpg_get_map kernel */

int dpg_reoptimize(dpg_ctx* ctx, int64_t n_nodes, const int32_t* pass_numbers, const float* est_poses,
                   const float* odom_only, const dpg_icp_params* icp_params, const dpg_gn_params* gn_params,
                   const dpg_reopt_params* params, double* poses_out, dpg_reopt_stats* stats);

/* DpgSLAM::reoptimize for a live incremental graph g (dpg_slam.cc:35-120): the sweep of
 * dpg_reoptimize (candidates, ONE batched ICP, the factors in the reference's order: pass prior or
 * odometry per node, every successive alignment, the converged loop closures) on g's context, then g
 * is rebuilt from exactly those factors -- dpg_inc_reset + ONE dpg_inc_update of all V nodes from
 * est_poses: the reference's new ISAM2 + new graph_ and its one update (:36-39, :111-119), under g's
 * own update semantics (DPG_INC_ISAM2: one step; DPG_INC_BATCH: to convergence).  Later
 * dpg_add_node calls then build on the swept graph, as the reference's per-node updates do after
 * reoptimize.  The context's scan store must hold the V nodes (it does after V dpg_add_node).
 * poses_out[V][3] = g's estimate; stats.gn carries the update's iterations and error. */
struct dpg_inc;
int dpg_reoptimize_inc(struct dpg_inc* g, int64_t n_nodes, const int32_t* pass_numbers, const float* est_poses,
                       const float* odom_only, const dpg_icp_params* icp_params, const dpg_reopt_params* params,
                       double* poses_out, dpg_reopt_stats* stats);

/* ---- incremental per-node solve (updatePoseGraphObsConstraints -> optimizeGraph -> isam_->update,
 *      dpg_slam.cc:255-329, ISAM2 built at :22 with default parameters) ----
 * A device-resident pose graph that grows by one isam_->update per call.  The elimination order of
 * the Cholesky is kept and extended (new nodes at its end, new edges add their fill along the
 * elimination tree); a fresh minimum-degree order is computed every reorder_every nodes or when the
 * fill grows 1.5x.  DPG_INC_ISAM2: ISAM2 semantics with its defaults (relinearize variables whose
 * max |delta| >= 0.1 on every 10th update, one Gauss-Newton step from the linearization point per
 * update; exact solve instead of the 0.001 wildfire threshold).  DPG_INC_BATCH: Gauss-Newton to
 * convergence on every update.  duplicate_factors = 1 reproduces SURVEY Q1 (the reference re-adds
 * the whole accumulated graph_ on every update: a factor's information is scaled by the number of
 * updates it has been part of). */
#define DPG_INC_ISAM2 0
#define DPG_INC_BATCH 1
typedef struct dpg_inc_params {
    int32_t mode;                    /* DPG_INC_ISAM2 | DPG_INC_BATCH */
    int32_t relinearize_skip;        /* 10 (ISAM2Params::relinearizeSkip) */
    double relinearize_threshold;    /* 0.1 (ISAM2Params::relinearizeThreshold) */
    int32_t duplicate_factors;       /* 0; 1: SURVEY Q1 */
    int32_t reorder_every;           /* 32: a fresh fill-reducing order every this many new nodes */
    int32_t reorder_lead;            /* 8: that order is computed on a worker thread from a snapshot of
                                        the graph this many nodes before it is due, then extended by the
                                        nodes and edges that arrived since; 0: on the calling thread */
    int32_t full_refactor;           /* 0: ISAM2 updates refactor only the fronts the update touches
                                        (new nodes, new factors' and pairs' nodes, structure changes,
                                        and everything above them) -- isam_->update's partial
                                        re-elimination, bit-identical to a full refactorization;
                                        1: every front, every update */
    dpg_gn_params gn;                /* DPG_INC_BATCH: the Gauss-Newton loop (Cholesky) */
} dpg_inc_params;

typedef struct dpg_inc_stats {
    int64_t n_nodes, n_factors;
    int64_t nnz_l;                   /* 3x3 blocks below the diagonal of L */
    int32_t reordered;               /* 1: this update computed a fresh order */
    int32_t relinearized;            /* ISAM2: variables relinearized by this update */
    int32_t gn_iterations;           /* ISAM2: 1 */
    int32_t fronts_kept;             /* ISAM2: Cholesky fronts this update kept from the last one
                                        (0: a full refactorization) */
    double error;                    /* 0.5 chi2 at the last linearization point */
    double last_delta_inf;
    double ms_total, ms_symbolic, ms_numeric;
} dpg_inc_stats;

typedef struct dpg_inc dpg_inc;
void dpg_inc_params_default(dpg_inc_params* p);
dpg_inc* dpg_inc_create(dpg_ctx* ctx, const dpg_inc_params* params);
void dpg_inc_destroy(dpg_inc* g);
/* reoptimize() (dpg_slam.cc:36-39): a new ISAM2 and a new graph */
int dpg_inc_reset(dpg_inc* g);
/* isam_->update(new factors, new values): n_new nodes appended (keys V .. V+n_new-1, initial values
 * init[n_new][3]) and the factors added since the last update (keys < V + n_new). */
int dpg_inc_update(dpg_inc* g, int64_t n_new, const double* init, const dpg_factor* factors, int64_t n_factors,
                   dpg_inc_stats* stats);
int64_t dpg_inc_num_nodes(const dpg_inc* g);
/* calculateEstimate() of the first n nodes: poses[n][3] */
int dpg_inc_get_poses(dpg_inc* g, double* poses, int64_t n);
/* ISAM2::marginalCovariance: cov_out[n][9] from the incremental graph's factor as it stands (the
 * conventions and errors of dpg_gn_marginals; nodes == NULL: every node, n = dpg_inc_num_nodes).
 * Nothing is re-linearized or refactored, and L, the state kept for the next partial
 * re-elimination and the estimates are untouched: updates interleaved with marginals calls give
 * bitwise the estimates of updates without them.
 * DPG_INC_ISAM2: the covariance at the linearization points theta that dpg_inc_export returns
 * (ISAM2's own behaviour: not at the estimate).  DPG_INC_BATCH: at the point of the last update's
 * last factorization (its last Gauss-Newton iterations may be chord steps).  With
 * duplicate_factors = 1 the multiplicities are part of H.
 * DPG_ERR_STATE also: before the first update, after a failed update or dpg_inc_load until the
 * next successful update. */
int dpg_inc_marginals(dpg_inc* g, const int32_t* nodes, int64_t n, double* cov_out /*[n][9]*/);
/* dpg_gn_cross_covariances / dpg_gn_joint_marginal / dpg_gn_relative_covariances on the incremental
 * graph's factor as it stands: the conventions, the read-only guarantee and the errors of
 * dpg_inc_marginals (DPG_ERR_ARG also for a NULL list with n > 0).  The relative-pose Jacobian is
 * taken at theta, the point the factor was linearized at. */
int dpg_inc_cross_covariances(dpg_inc* g, const int32_t* pairs /*[n][2]*/, int64_t n, double* cov_out /*[n][9]*/);
int dpg_inc_joint_marginal(dpg_inc* g, const int32_t* nodes, int64_t n, double* cov_out /*[3n][3n] row-major*/);
int dpg_inc_relative_covariances(dpg_inc* g, const int32_t* pairs /*[n][2]*/, int64_t n, double* cov_out /*[n][9]*/);

/* Graph checkpoint ("optional binary dump of the graph (poses, edges,
 * measurements)"; the reference keeps dpg_nodes_ with their scans, graph_ and isam_ only in memory,
 * dpg_slam.h:362,367,372).  dpg_inc_save writes the graph's factors, node pairs (arrival order),
 * linearization points, estimate, per-variable |delta|, update count and parameters, and the
 * context's scan store (full clouds, downsample ratio) when it holds the graph's nodes (the
 * dpg_add_node path; a graph fed by dpg_inc_update alone is saved without scans), to one binary
 * file.  dpg_inc_load restores it on ctx (single device; a saved scan store replaces ctx's and is
 * indexed, else ctx's store is left as it is): the next
 * dpg_add_node / dpg_inc_update continues the saved run, ISAM2's relinearization schedule
 * included; the elimination order is recomputed from the saved pattern, so later estimates agree
 * with an uninterrupted run to rounding.  dpg_inc_load returns NULL on error (dpg_last_error);
 * a file of another version or layout is rejected. */
int dpg_inc_save(dpg_inc* g, const char* path);
dpg_inc* dpg_inc_load(dpg_ctx* ctx, const char* path);
/* The graph's state as host copies (the checkpoint's arrays without the scans): the update count,
 * the factors and the update that added each (up to cap_factors of them), the linearization points
 * theta [3 V], the estimate [3 V] and the last max |delta| per node [V] (V = dpg_inc_num_nodes);
 * any pointer may be NULL.  Returns the number of factors, negative on error. */
int64_t dpg_inc_export(dpg_inc* g, int64_t* updates, dpg_factor* factors, int32_t* created, int64_t cap_factors,
                       double* theta, double* est, double* maxd);

/* Append nodes to the uploaded scan store (dpg_scans_upload's layout): pts_xy = the new nodes' full
 * clouds concatenated, node_offsets[n_new + 1] relative to pts_xy; the downsample ratio must match
 * the store's.  Only the new nodes' neighbour indexes are built. */
int dpg_scans_append(dpg_ctx* ctx, const float* pts_xy, const int64_t* node_offsets, int64_t n_new,
                     int32_t downsample_ratio);

typedef struct dpg_add_node_stats {
    int64_t n_icp_edges;             /* successive + loop-closure alignments run for this node */
    int64_t n_loop_closures;         /* loop-closure factors added (converged alignments) */
    double ms_icp;                   /* batched ICP of the node's edges (incl. its index build) */
    dpg_inc_stats update;
} dpg_add_node_stats;

/* One new node (id V = dpg_inc_num_nodes(g)) with explicit alignments: the node's base_link cloud
 * joins the scan store; ONE batched ICP aligns the successive pair (V-1, V) when `successive` and
 * every pair in pairs[n_pairs][2] = {node_1 (target), node_2 (source)}, keys <= V; the successive
 * factor always joins the graph, the other pairs' factors when converged (dpg_slam.cc:263-267,
 * 295-301), after the caller's `extra` factors, in one dpg_inc_update (initial pose init_pose).
 * The update's symbolic work runs on the host while the GPU aligns, with every pair in the pattern:
 * a pair whose alignment does not converge stays an explicit zero block of H (no factor; the
 * solution is unchanged, the update's nnz statistics count it). */
int dpg_add_node_pairs(dpg_inc* g, const float* cloud_xy, int64_t n_pts, const float init_pose[3],
                       const dpg_factor* extra, int64_t n_extra, const int32_t* pairs, int64_t n_pairs,
                       int32_t successive, const dpg_icp_params* icp_params, dpg_add_node_stats* stats);
/* One new node, as updatePoseGraphObsConstraints + optimizeGraph run it (dpg_slam.cc:255-314):
 * the node's base_link cloud is appended to the scan store (node id = dpg_inc_num_nodes(g)); ONE
 * batched ICP aligns the successive pair (prev, new) and every loop-closure candidate (i, prev),
 * i < V - 2 (V = nodes before this one), whose float distance to prev's estimate is within
 * max_node_dist_within_pass (same pass_numbers) or max_node_dist_across_passes; the successive
 * factor is always added, loop closures when converged; together with the caller's `extra`
 * factors (the pass prior or the odometry Between) they go into one dpg_inc_update with the node's
 * initial pose init_pose (createRelativePositionedNode, float).  pass_numbers[V + 1]: every node's
 * pass, the new one last.  non_successive = 0 skips the loop closures
 * (non_successive_scan_constraints_, parameters.h:349-354).  The ICP guesses use the estimates of
 * dpg_inc_get_poses rounded to float (the reference's dpg_nodes_ positions are float). */
int dpg_add_node(dpg_inc* g, const float* cloud_xy, int64_t n_pts, const int32_t* pass_numbers, const float init_pose[3],
                 const dpg_factor* extra, int64_t n_extra, const dpg_icp_params* icp_params,
                 const dpg_reopt_params* params, int32_t non_successive, dpg_add_node_stats* stats);

/* ---- DPG change detection (DpgSLAM::executeDPG, dpg_slam.cc:865-886) ----
 * The dynamic node state (DpgNode/Measurement: per-beam label and sector, per-node sector
 * activation and active flag) lives on the device in a dpg_dpg store; executeDPG runs on it.
 * Semantics are the reference's with its Q8 defects fixed ("DPG"): a grid point is
 * transformed into the map frame once; unlabelled points count as STATIC; the uncovered-cell set
 * loses every cell the candidate covers; the bin ratio is a real division; the bin score uses the
 * pose-chain node whose grid is tested and its own scan's angle range; removed points are labelled
 * on their own node; a deactivated sector skips one removed point (continue, not break); the pose
 * chain is placed at the nodes' CURRENT estimates (est_poses) everywhere -- the reference's
 * current_pass_nodes_ holds by-value DpgNode copies made at creation (dpg_slam.cc:195,307,598,
 * dpg_node.h:163) that optimizeGraph never updates, so its chain grids and proximity search sit at
 * creation-time poses while its bin score (:793-800) and sector update (:893-898) use the
 * optimised ones (DPG item 8). */
enum { DPG_LABEL_STATIC = 0, DPG_LABEL_ADDED = 1, DPG_LABEL_REMOVED = 2, DPG_LABEL_NOT_YET_LABELED = 3,
       DPG_LABEL_MAX_RANGE = 4 };   /* PointLabel, dpg_measurement.h:21 */

typedef struct dpg_change_params {
    int32_t num_sectors;                        /* 5 (parameters.h:44) */
    int32_t current_pose_chain_len;             /* 5 (parameters.h:57), <= 15 */
    int32_t num_bins_for_change_detection;      /* uninitialised in the reference (parameters.h:62); 36 */
    int32_t pad;
    double delta_change_threshold;              /* 0.20 (parameters.h:67) */
    double current_pose_graph_coverage_threshold; /* 1.0 (parameters.h:72) */
    double occ_grid_resolution;                 /* 0.05 (parameters.h:77) */
    float minimum_percent_active_sectors;       /* 0.5 (parameters.h:82) */
    float distance_threshold_for_local_submap_nodes; /* 5.0 (parameters.h:87) */
    float laser[3];                             /* laser pose in base_link: 0.2, 0, 0 (parameters.h:319-339) */
    float pad2;
} dpg_change_params;

typedef struct dpg_change_stats {
    int64_t n_chain;            /* current pose chain length used */
    int64_t n_candidates;       /* active past nodes within the proximity threshold */
    int64_t n_submap_nodes;     /* candidates merged into the local submap */
    int64_t n_chain_cells;      /* cells of the pose-chain grids (the uncovered set at the start) */
    int64_t n_uncovered;        /* chain cells left uncovered by the submap */
    int64_t n_added;            /* points labelled ADDED (committed nodes only) */
    int64_t n_removed;          /* distinct points labelled REMOVED */
    int64_t n_committed;        /* pose-chain nodes whose bin score passed */
    int64_t n_sectors_deactivated; /* by updateNodesAndSectorStatus */
    int64_t n_nodes_deactivated;
    int64_t grid_cells;         /* dense window cells (W x H) */
    int64_t n_samples;          /* ray samples marched (all rasterisation passes) */
    double ms_total;            /* wall time of dpg_execute_dpg */
    double ms_kernels;          /* device time, HIP events around the device work */
} dpg_change_stats;

typedef struct dpg_dpg dpg_dpg;

void dpg_change_params_default(dpg_change_params* p);
/* Node store: n_nodes scans (ranges[beam_offsets[v] .. beam_offsets[v+1]), geom[v] = angle_min,
 * angle_max, range_max).  Labels start as MeasurementPoint's constructor sets them
 * (dpg_measurement.h:41-46), sectors as createNode numbers them (dpg_slam.cc:499-507), every sector
 * and node active.  NULL on error (dpg_last_error). */
dpg_dpg* dpg_dpg_create(dpg_ctx* ctx, int64_t n_nodes, const int64_t* beam_offsets, const float* ranges,
                        const float* geom /*[V][3]*/, const dpg_change_params* params);
void dpg_dpg_destroy(dpg_dpg* d);
/* Add n_new nodes' scans at the end (createNode of each new node, dpg_slam.cc:488-513):
 * beam_offsets[n_new + 1] relative to ranges[0]; existing labels, sectors and activity are kept. */
int dpg_dpg_append(dpg_dpg* d, int64_t n_new, const int64_t* beam_offsets, const float* ranges,
                   const float* geom /*[n_new][3]*/);
/* executeDPG after node n_nodes-1 was added: dpg_nodes_ = nodes [0, n_nodes), current_pass_nodes_ =
 * the last current_pass_len of them; est_poses[n_nodes][3] the estimated node poses. */
int dpg_execute_dpg(dpg_dpg* d, int64_t n_nodes, int64_t current_pass_len, const float* est_poses,
                    dpg_change_stats* stats);
/* The same with the pose chain placed where the reference places it: chain_poses[chain_n][3] are the
 * poses of the last chain_n = min(current_pass_len, current_pose_chain_len) nodes as the host's
 * current_pass_nodes_ copies hold them (dpg_slam.cc:195,307,598: by-value copies taken at creation
 * and never refreshed by optimizeGraph).  They place the chain grids (computeLocalSubMap,
 * :591-620) and the submap proximity search (:646-668); the bin score (:786-800) and the sector
 * update (:893-898) keep est_poses, as dpg_nodes_ does.  chain_poses == NULL is dpg_execute_dpg
 * (every use at est_poses, Q8 fix 8 of DESIGN.md section 3). */
int dpg_execute_dpg_chain(dpg_dpg* d, int64_t n_nodes, int64_t current_pass_len, const float* est_poses,
                          const float* chain_poses, dpg_change_stats* stats);
/* Copy the node state back (any pointer may be NULL): labels[B], sector_active[V] (bit s = sector s
 * active), node_active[V]. */
int dpg_dpg_fetch(dpg_dpg* d, uint8_t* labels, uint8_t* sector_active, uint8_t* node_active);
/* Overwrite the node state (tests, checkpoint restore); NULL leaves that part unchanged. */
int dpg_dpg_load(dpg_dpg* d, const uint8_t* labels, const uint8_t* sector_active, const uint8_t* node_active);
/* DpgSLAM::getActiveAndDynamicMapPoints (dpg_slam.cc:832-863) over nodes [0, n_nodes): the four
 * point lists in node/beam order, concatenated into out[cap][2] as active_static | active_added |
 * dynamic_removed | dynamic_added; counts[4] receives their sizes.  Returns the total (negative:
 * error); writes nothing past cap. */
int64_t dpg_active_dynamic_points(dpg_dpg* d, int64_t n_nodes, const float* est_poses, float* out,
                                  int64_t cap, int64_t counts[4]);

/* ---- Occupancy grid of the active pose graph (nav_msgs/OccupancyGrid: free, occupied, unknown) ----
 * The counting form of the change detection's rasteriser over every active node of [0, n_nodes) at
 * est_poses, at a resolution of its own.
 *   Included beams: exactly the beams executeDPG rasterises -- the node is active and the beam's
 *     sector is active.
 *   Cell key of a coordinate v: round((double)v / res), C round (halves away from zero).
 *   Free samples of a beam with lidar position f (the node's lidar in the map) and end point m:
 *     nbins = (uint32)round((double)range / res), inc = (float)(1.0 / (double)nbins), t = 0.0f;
 *     while ((double)t < 1.0) the sample is ((1 - t) * f.x + t * m.x, (1 - t) * f.y + t * m.y) in float
 *     without contraction, then t = t + inc (getIntermediateFreeCellsInFOV, dpg_slam.cc:1059-1082).
 *   hits[c]:   included beams whose label is neither DPG_LABEL_MAX_RANGE nor DPG_LABEL_REMOVED and
 *     whose end point m falls in cell c.
 *   misses[c]: free samples of included beams (every label) that fall in c, except a sample in its
 *     own beam's end-point cell when that end point counted as a hit (otherwise every wall cell would
 *     read about 50 %).
 *   occ[c]: with n = hits + misses, -1 when n == 0, else (200 * hits + n) / (2 * n) in integer
 *     arithmetic: 100 * hits / n rounded half up, 0..100.
 *   Box (host, fp64, over the active nodes; r_v = the node's largest range, (lx_v, ly_v) its lidar):
 *     x0 = floor(min_v(lx_v - r_v) / res) - margin, x1 = ceil(max_v(lx_v + r_v) / res) + margin,
 *     y0, y1 alike, w = x1 - x0 + 1, h = y1 - y0 + 1; no active node: w = h = 0 and the call succeeds.
 *     Cell (ix, iy) has key (x0 + ix, y0 + iy); the arrays are row-major [h][w]; the lower-left corner
 *     of cell (0, 0) lies at ((x0 - 0.5) * res, (y0 - 0.5) * res) in the map frame.
 * All accumulation is integer and order-free: two calls on the same state are bitwise equal.  The
 * call reads the store and refreshes its cached node frames, nothing else: labels, sectors, activity,
 * the change-detection window and its kept chain planes stay as they are.  Its device buffers are its
 * own, allocated at the first request and regrown only when a request needs more. */
typedef struct dpg_grid_params {
    double resolution;     /* m per cell; 0 = the store's occ_grid_resolution */
    int64_t max_cells;     /* 0 = 1 << 25 (also the largest value); a larger box is DPG_ERR_SIZE */
    int32_t margin_cells;  /* default 1 */
    int32_t pad;           /* 0; 1..9 run a measurement variant of the raster kernel (same result,
                              DESIGN.md K7, tools/occ_grid_probe.py) */
} dpg_grid_params;

typedef struct dpg_grid_info {
    int32_t x0, y0, w, h;
    double resolution;
    int64_t n_nodes_used;  /* active nodes */
    int64_t n_beams_used;  /* included beams */
    int64_t n_hits;        /* sum of hits[] */
    int64_t n_samples;     /* free samples marched (those dropped in their beam's hit cell included) */
    int64_t n_oob;         /* end points and samples outside the box: 0 by construction */
    double ms_total, ms_kernels;
    int64_t n_direct;      /* adds that found no slot in a workgroup's LDS table and went straight to the global counter */
    int64_t n_flushed;     /* global atomic adds issued when the LDS tables were flushed */
} dpg_grid_info;

#define DPG_GRID_PARAMS_SIZE 24
#define DPG_GRID_INFO_SIZE 96
#ifdef __cplusplus
 static_assert(sizeof(dpg_grid_params) == DPG_GRID_PARAMS_SIZE && sizeof(dpg_grid_info) == DPG_GRID_INFO_SIZE, "grid ABI structs");
#else
 _Static_assert(sizeof(dpg_grid_params) == DPG_GRID_PARAMS_SIZE && sizeof(dpg_grid_info) == DPG_GRID_INFO_SIZE, "grid ABI structs");
#endif

void dpg_grid_params_default(dpg_grid_params* p);
/* The grid.  hits, misses [cap] int32 and occ [cap] int8 may each be NULL.  With all three NULL the
 * call only plans: info receives the box and nothing is launched.  Any non-NULL output with
 * cap < w * h is DPG_ERR_SIZE with nothing written.  info may be NULL. */
int dpg_occupancy_grid(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const dpg_grid_params* p,
                       int32_t* hits, int32_t* misses, int8_t* occ, int64_t cap, dpg_grid_info* info);
/* Each node's lidar position in the map frame, lidar_xy[n_nodes][2], and each beam's end point,
 * end_xy[B][2] with B = the beams of nodes [0, n_nodes), as the device computes them (every node and
 * beam, whatever its state).  Either pointer may be NULL; cap_beams < B with end_xy given is
 * DPG_ERR_SIZE with nothing written. */
int dpg_dpg_beam_geometry(dpg_dpg* d, int64_t n_nodes, const float* est_poses, float* lidar_xy, float* end_xy,
                          int64_t cap_beams);
/* Host: the occupancy byte of n cells from their counters (the formula above). */
void dpg_occupancy_from_counts(const int32_t* hits, const int32_t* misses, int64_t n, int8_t* occ);
/* Host: the box rule above over n nodes (lidar_xy[n][2], largest range r_v[n], active[n]; active ==
 * NULL: all): box = x0, y0, w, h.  DPG_ERR_ARG: res not a positive number, margin < 0 or a
 * non-finite input of an active node; DPG_ERR_SIZE: a cell key beyond +-2^29. */
int dpg_grid_box(const float* lidar_xy, const float* r_v, const uint8_t* active, int64_t n, double res,
                 int32_t margin, int32_t box[4]);

/* ---- correlative scan matching: a loop-closure guess that needs no good guess ----
 * Every alignment starts ICP from the pose estimates (dpg_icp_guess) and ICP's correspondence search
 * stops at icp_max_correspondence_distance, so a loop-closure candidate whose estimates drifted by
 * more than about that much fails its ICP.  dpg_csm_batch scores, per pair (target t, source s),
 * every pose in a window of (dx, dy, dtheta) around the guess against a smoothed raster of the target
 * scan (Olson 2009) and returns the best pose as the refined guess, which dpg_icp_batch_prepare_guess
 * hands to ICP.  The reference has no such stage.  After one float transform per point and angle all
 * work is integer, so every output is exact and order-free.
 *
 *   lut[d2], 0 <= d2 <= R^2 (R = kernel_radius): (uint8)floor(255 exp(-d2 res^2 / (2 sigma^2)) + 0.5),
 *     in double, res and sigma widened from float.  Non-increasing in d2.
 *   key of a coordinate v (float): round((double)v / res), C round, res widened from float -- the
 *     occupancy grid's rule.  A point with a non-finite coordinate or |(double)v / res| >= 2^29
 *     contributes nothing, as target and as source.
 *   Table T of node t, cell keys (u, v) in [-half_cells, half_cells]^2, in t's own frame, over the
 *     store's downsampled cloud of t: T[u, v] = max of lut[d2] over the target points whose key lies
 *     at squared cell distance d2 <= R^2 from (u, v); 0 when there is none.  A point whose own key lies
 *     outside the table still spreads into it.
 *   Rotations (dpg_csm_rotations): theta_g = atan2((double)guess[3], (double)guess[0]),
 *     angle_a = theta_g + (a - half_a) (double)angle_step, (c_a, s_a) = ((float)cos, (float)sin) of it,
 *     a = 0 .. 2 half_a.  The kernel receives this table and calls no trigonometric function.
 *   Source cell of point (x, y) at angle a, with (tx, ty) = (guess[2], guess[5]), in float, one
 *     rounding per operation: qx = ((c_a x) - (s_a y)) + tx, qy = ((s_a x) + (c_a y)) + ty;
 *     (kx, ky) = the keys of (qx, qy).
 *   score(a, dx, dy), |dx| <= half_x, |dy| <= half_y: the int32 sum over the source points of
 *     T[kx + dx, ky + dy], over the points whose shifted cell lies in the table.
 *   Winner: the highest score; ties by smaller |a - half_a|, then smaller dx^2 + dy^2, then smaller a,
 *     then smaller dy, then smaller dx.
 *   Refined guess rows: (c_a, -s_a, (float)((double)tx + dx (double)res)),
 *                       (s_a,  c_a, (float)((double)ty + dy (double)res)).
 * One workgroup per pair with the table in LDS.  Its working set must fit 160 KiB:
 *   dpg_csm_lds_bytes = round_up_16((2 half_cells + 1 + 4 half_x) (2 half_cells + 1 + 4 half_y))
 *                       + DPG_CSM_LDS_FIXED <= DPG_CSM_LDS_BUDGET
 * (the table with a zero apron of twice the window on every side, then a fixed part: one chunk of
 * packed source cells, the smoothing stencil, the reduction words). */
typedef struct dpg_csm_params {
    float resolution;       /* m per cell, default 0.1; finite, > 0 */
    float sigma;            /* smoothing, m, default 0.1; finite, > 0 */
    int32_t kernel_radius;  /* R, cells, default 3; 0 .. 7 */
    int32_t half_cells;     /* default 160; the table covers keys [-half_cells, half_cells]^2; >= 0 */
    int32_t half_x, half_y; /* translation window, cells, default 15, 15; 0 .. 64 */
    int32_t half_a;         /* angle window, steps, default 20; 0 .. 64 */
    float angle_step;       /* radians per step, default 0.5 degrees; finite, > 0 */
} dpg_csm_params;

#define DPG_CSM_OK 0
#define DPG_CSM_NO_OVERLAP 1   /* the best score is 0: no source point met the table anywhere in the window */
typedef struct dpg_csm_result {
    float guess[6];         /* the refined guess, rows as dpg_icp_guess writes them */
    int32_t score;          /* the winner's score */
    int32_t score_at_guess; /* score(half_a, 0, 0) */
    int32_t n_src;          /* points of the source cloud: the largest possible score is 255 n_src */
    int32_t best_a, best_dx, best_dy;   /* the winner: a in 0 .. 2 half_a, dx, dy in cells */
    int32_t status;         /* DPG_CSM_* */
    int32_t pad[3];
} dpg_csm_result;

#define DPG_CSM_PARAMS_SIZE 32
#define DPG_CSM_RESULT_SIZE 64
#define DPG_CSM_LDS_FIXED 9536
#define DPG_CSM_LDS_BUDGET 163840
#ifdef __cplusplus
 static_assert(sizeof(dpg_csm_params) == DPG_CSM_PARAMS_SIZE && sizeof(dpg_csm_result) == DPG_CSM_RESULT_SIZE, "csm ABI structs");
#else
 _Static_assert(sizeof(dpg_csm_params) == DPG_CSM_PARAMS_SIZE && sizeof(dpg_csm_result) == DPG_CSM_RESULT_SIZE, "csm ABI structs");
#endif

void dpg_csm_params_default(dpg_csm_params* p);
/* Host.  The kernel's LDS bytes by the formula above; DPG_ERR_ARG for an invalid field or a working
 * set above DPG_CSM_LDS_BUDGET (every dpg_csm_* call checks its params through this). */
int64_t dpg_csm_lds_bytes(const dpg_csm_params* p);
/* Host.  lut_out[R * R + 1]; for the defaults 255, 155, 94, 57, 35, 21, 13, 8, 5, 3. */
int dpg_csm_lut(const dpg_csm_params* p, uint8_t* lut_out);
/* Host.  rot_out[2 half_a + 1][2] = (c_a, s_a). */
int dpg_csm_rotations(const float guess[6], const dpg_csm_params* p, float* rot_out);
/* The match of n_edges pairs, edges[e] = {target, source} over the uploaded scan store, on the context
 * stream; blocks until results_out[n_edges] is written.  Exactly one of poses ([V][3], turned into
 * guesses by dpg_icp_guess as dpg_icp_batch_prepare does) and guesses ([n_edges][6]) is given.
 * Errors: DPG_ERR_ARG -- params, an edge naming a missing node, both or neither of poses / guesses;
 * DPG_ERR_STATE -- no scans uploaded, or a multi-device, virtual or rank context; DPG_ERR_SIZE, with
 * nothing written -- cap < n_edges. */
int dpg_csm_batch(dpg_ctx* ctx, const int32_t* edges, int64_t n_edges, const float* poses, const float* guesses,
                  const dpg_csm_params* params, dpg_csm_result* results_out, int64_t cap);
/* Diagnostic: the table of one node as the kernel built it, (2 half_cells + 1)^2 bytes, row-major
 * with v outer; cap in bytes, DPG_ERR_SIZE when smaller. */
int dpg_csm_table(dpg_ctx* ctx, int32_t node, const dpg_csm_params* params, uint8_t* out, int64_t cap);
/* Diagnostic: the full score volume of one pair from the same kernel, out[2 half_a + 1][2 half_y + 1]
 * [2 half_x + 1]; cap in int32 elements, DPG_ERR_SIZE when smaller. */
int dpg_csm_scores(dpg_ctx* ctx, int32_t target, int32_t source, const float guess[6], const dpg_csm_params* params,
                   int32_t* out, int64_t cap);
/* Device time of the last dpg_csm_batch / _table / _scores kernel (ms, HIP events); < 0 before one. */
float dpg_csm_kernel_ms(dpg_ctx* ctx);
/* dpg_icp_batch_prepare with the guess of every edge given (guesses[n_edges][6], rows as
 * dpg_icp_guess writes them) instead of derived from poses; dpg_icp_batch_run / _fetch follow unchanged. */
int dpg_icp_batch_prepare_guess(dpg_ctx* ctx, const int32_t* edges, int64_t n_edges, const float* guesses,
                                const dpg_icp_params* params);

/* ---- loop-closure verification: is an alignment consistent with what both scans saw through? ----
 * ICP reports `converged` for an alignment that slid into a wrong local minimum too, and every
 * converged loop closure becomes a factor.  dpg_verify_batch checks an alignment T of a pair (target t,
 * source s) by free-space consistency (Olson's and Cartographer's visibility test): where t's scan
 * looked through a cell to something behind it, s's scan placed by T must have no return, and the
 * reverse.  It needs nothing but the two clouds of the scan store and T.  The reference has no such
 * stage.  After one float transform per point all work is integer, so every output is exact and
 * independent of point order.
 *
 *   key of a coordinate v (float): round((double)v / res), C round, res widened from float -- the scan
 *     matcher's rule.  A point with a non-finite coordinate or |(double)v / res| >= 2^29 contributes
 *     nothing, as model and as moving point.
 *   Sensor key a = (ax, ay): the key of `sensor`, the lidar's position in the cloud's own frame;
 *     |ax|, |ay| <= half_cells (H).
 *   Table of a model cloud, cell keys in [-H, H]^2 in the cloud's own frame, from two sets of cells:
 *     OCC: every table cell at squared cell distance <= occ_radius^2 (R) from the key of a valid model
 *       point.  A point whose own key lies outside the table still spreads into it.
 *     FREE: for every valid model point with key b, d = b - a and n = max(|dx|, |dy|): the cells
 *       a + (off(dx, n, i), off(dy, n, i)), i = 0 .. n - 1, that lie in the table, where
 *       off(d, n, i) = sign(d) floor((2 i |d| + n) / (2 n)) in 64-bit integers (i d / n rounded half
 *       up in magnitude).  The end cell i = n is not marked; n = 0 marks nothing.  Along the longer
 *       axis off = i, and |ax|, |ay| <= H, so every cell with i > 2H lies outside the table: the loop
 *       may stop at min(n, 2H + 1) with the same result, and does.
 *     State of a cell: 2 if in OCC, else 1 if in FREE, else 0.  Occupied wins.
 *   Moving points under T (rows as dpg_icp_result.T / dpg_icp_guess write them): c = T[0], s = T[3],
 *     tx = T[2], ty = T[5], as they stand (not normalised), in float, one rounding per operation.
 *     Direction 0, a source point (x, y) into the target's frame against the target's table:
 *       qx = ((c x) - (s y)) + tx, qy = ((s x) + (c y)) + ty.
 *     Direction 1, a target point into the source's frame against the source's table:
 *       dx = x - tx, dy = y - ty, qx = (c dx) + (s dy), qy = (c dy) - (s dx).
 *   Counts per direction d: n_pts[d] the points of the moving cloud; n_in[d] its valid points whose
 *     key lies in the table; n_support[d] those of n_in[d] on state 2; n_free[d] those on state 1;
 *     the rest of n_in[d] is unknown.
 * One workgroup per (pair, direction) with the model's table in LDS as two bit planes (OCC, FREE):
 *   dpg_verify_lds_bytes = 2 round_up_16(4 ceil((2 half_cells + 1)^2 / 32)) + DPG_VERIFY_LDS_FIXED
 *                          <= DPG_VERIFY_LDS_BUDGET
 * (the fixed part: one chunk of model keys, the counters). */
typedef struct dpg_verify_params {
    float resolution;       /* m per cell, default 0.1; finite, > 0 */
    int32_t half_cells;     /* H, default 160; the table covers keys [-H, H]^2; >= 0 */
    int32_t occ_radius;     /* R, cells, default 2; 0 .. 7 */
    float sensor[2];        /* the lidar in the cloud's frame, default (0.2, 0): dpg_store_params.laser; finite, key within the table */
    int32_t pad[3];
} dpg_verify_params;

#define DPG_VERIFY_OK 0
#define DPG_VERIFY_NO_OVERLAP 1   /* n_in[0] == 0 || n_in[1] == 0: a direction has no point on the other's table */
typedef struct dpg_verify_result {
    int32_t n_pts[2], n_in[2], n_support[2], n_free[2];   /* [direction] */
    int32_t status;         /* DPG_VERIFY_* */
    int32_t pad[7];
} dpg_verify_result;

#define DPG_VERIFY_PARAMS_SIZE 32
#define DPG_VERIFY_RESULT_SIZE 64
#define DPG_VERIFY_LDS_FIXED 4160
#define DPG_VERIFY_LDS_BUDGET 163840
#ifdef __cplusplus
 static_assert(sizeof(dpg_verify_params) == DPG_VERIFY_PARAMS_SIZE && sizeof(dpg_verify_result) == DPG_VERIFY_RESULT_SIZE, "verify ABI structs");
#else
 _Static_assert(sizeof(dpg_verify_params) == DPG_VERIFY_PARAMS_SIZE && sizeof(dpg_verify_result) == DPG_VERIFY_RESULT_SIZE, "verify ABI structs");
#endif

void dpg_verify_params_default(dpg_verify_params* p);
/* Host.  DPG_OK, or DPG_ERR_ARG for a field outside its range, a non-finite sensor or a sensor key
 * outside the table. */
int dpg_verify_params_check(const dpg_verify_params* p);
/* Host.  The kernel's LDS bytes by the formula above; DPG_ERR_ARG for params that fail the check or a
 * working set above DPG_VERIFY_LDS_BUDGET (every dpg_verify_* call checks its params through this). */
int64_t dpg_verify_lds_bytes(const dpg_verify_params* p);
/* Host.  key[2] = the sensor key (ax, ay). */
int dpg_verify_sensor_key(const dpg_verify_params* p, int32_t key[2]);
/* The check of n_edges alignments, edges[e] = {target, source} over the uploaded scan store with
 * transforms[e][6] (typically dpg_icp_result.T of that pair), on the context stream: one upload, one
 * launch (both directions of every pair), one copy back; blocks until results_out[n_edges] is
 * written.  n_edges = 0 launches nothing.  Errors, each raised before anything is launched or
 * written: DPG_ERR_ARG -- params, an edge naming a missing node; DPG_ERR_STATE -- no scans uploaded,
 * or a multi-device, virtual or rank context; DPG_ERR_SIZE -- cap < n_edges. */
int dpg_verify_batch(dpg_ctx* ctx, const int32_t* edges, int64_t n_edges, const float* transforms,
                     const dpg_verify_params* params, dpg_verify_result* results_out, int64_t cap);
/* Diagnostic: the state bytes (0 / 1 / 2) of one node's table as the kernel built it,
 * (2 half_cells + 1)^2 bytes, row-major with v outer; cap in bytes, DPG_ERR_SIZE when smaller. */
int dpg_verify_table(dpg_ctx* ctx, int32_t node, const dpg_verify_params* params, uint8_t* out, int64_t cap);
/* Device time of the last dpg_verify_batch / _table kernel (ms, HIP events); < 0 before one. */
float dpg_verify_kernel_ms(dpg_ctx* ctx);

/* ---- localisation of one scan in the active map: where a pass starts ----
 * The first node of every pass is created at (0, 0, 0) (createNewPassFirstNode), so a pass has to
 * begin where pass 0 began.  dpg_map_localize matches ONE scan against the whole active map -- the
 * occupancy grid of the store, smoothed into a likelihood field -- over a window that may be as
 * large as the map and the full circle, and returns the best pose.  The pair matcher above cannot do
 * this: it needs a target node and its table lives in LDS.  The reference has no such stage.  After
 * one float transform per point and angle all work is integer, so every output is exact and
 * order-free, and the pruned search returns what the exhaustive one returns.
 *
 *   res: params.resolution, or the store's occ_grid_resolution when 0 (double).
 *   Box (x0, y0, w, h) and occ: those of dpg_occupancy_grid(d, n_nodes, est_poses) for the same
 *     resolution / margin_cells / max_cells (pad = 0).
 *   lut[d2], 0 <= d2 <= R^2 (R = kernel_radius): dpg_csm_lut's bytes for ((float)res, sigma, R).
 *   Field F, uint8 [h][w]: a cell is occupied when occ >= occupied_min (1..100, so unknown never
 *     counts).  F[c] = the largest lut[d2] over the occupied cells of the box at squared cell
 *     distance d2 <= R^2 from c; 0 when there is none.  Outside the box F reads 0 and is not stored.
 *   Pooled field P, s = 1 << coarse_shift: P[x, y] = the largest F[x + i, y + j], 0 <= i, j < s, for
 *     x in [-(s - 1), w - 1] and y in [-(s - 1), h - 1] (stored [h + s - 1][w + s - 1], index
 *     (y + s - 1, x + s - 1)); 0 elsewhere.  P at (x, y) bounds F at every shift of an s x s block.
 *   Rotations (dpg_loc_rotations): angle_a = (double)guess_theta + (a - half_a) (double)angle_step,
 *     (c_a, s_a) = ((float)cos, (float)sin) of it, a = 0 .. 2 half_a.  No kernel calls a
 *     transcendental.
 *   Key of point (x, y) at angle a: rx = (c_a x) - (s_a y), ry = (s_a x) + (c_a y) in float, one
 *     rounding per operation; (kx, ky) = round((double)rx / res), round((double)ry / res), C round.
 *     A point with a non-finite coordinate or |v / res| >= 2^29 contributes nothing.
 *   (cx, cy) = the keys of (guess_x, guess_y); an invalid key is DPG_ERR_ARG.
 *   score(a, dx, dy), |dx| <= half_x, |dy| <= half_y: the int32 sum over the points of
 *     F[kx + cx + dx - x0, ky + cy + dy - y0].
 *   Blocks: nbx = ceil((2 half_x + 1) / s), nby alike.  Block (bx, by) covers dx = -half_x + bx s + i,
 *     dy = -half_y + by s + j, i, j < s, clipped to the window.  bound(a, bx, by) = the sum over the
 *     points of P at the block's first shift (i = j = 0), so bound >= score for every candidate of the
 *     block, exactly.
 *   Winner: the highest score; ties by smaller |a - half_a|, then smaller dx^2 + dy^2, then smaller a,
 *     then smaller dy, then smaller dx (the scan matcher's order).
 *   Pose: x = (float)((double)(cx + dx) res), y alike, theta = (float)angle_a; rot = (c_a, s_a).
 *   Search:
 *     1. every block's bound;
 *     2. seeds: per angle the block with the highest bound; ties by the smaller
 *        (2 dx0 + s - 1)^2 + (2 dy0 + s - 1)^2 ((dx0, dy0) the block's first shift: twice its centre's
 *        distance from the window's centre), then smaller by, then smaller bx;
 *     3. the seeds' candidates scored exactly; best0 = the best of them;
 *     4. frontier: every block with bound >= best0 (>=, so that the tie order survives);
 *     5. the frontier's candidates scored exactly; the winner is taken over seeds and frontier;
 *     6. a frontier of more than max_refine_blocks blocks: the call succeeds, returns the seeds'
 *        winner with DPG_LOC_UNPROVEN, and n_frontier reports the frontier's size.
 *     coarse_shift = 0 is the exhaustive search (a block is a candidate).
 *   Status: DPG_LOC_NO_OVERLAP when the returned score is 0 and either every seed's bound is 0 (then
 *     every score is 0) or the frontier was refined; else DPG_LOC_UNPROVEN when the frontier
 *     overflowed; else DPG_LOC_OK.  No active node (w = h = 0) succeeds with DPG_LOC_NO_OVERLAP.
 *   Sizes: n_pts <= 2^23 (255 n_pts fits int32); (2 half_a + 1) nbx nby and (2 half_a + 1) n_pts at
 *     most 2^29 each (DPG_ERR_SIZE beyond: the bound volume and the key table are device arrays), and
 *     min(max_refine_blocks, blocks) s^2 at most 2^36 (one launch scores the frontier).
 * The field is rebuilt by every call (a dpg_fmap, below, keeps one).  The call reads the store as dpg_occupancy_grid does and writes
 * nothing of executeDPG's state or of the grid's outputs; F, P and the search buffers belong to the
 * store, allocated at first use and regrown only for a larger request. */
typedef struct dpg_loc_params {
    double resolution;          /* m per cell; 0 = the store's occ_grid_resolution */
    int64_t max_cells;          /* as dpg_grid_params */
    int32_t margin_cells;       /* as dpg_grid_params, default 1 */
    float sigma;                /* smoothing, m, default 0.1; finite, > 0 */
    int32_t kernel_radius;      /* R, cells, default 3; 0 .. 7 */
    int32_t occupied_min;       /* default 50; 1 .. 100 */
    int32_t half_x, half_y;     /* translation window, cells, default 40, 40; 0 .. 2^15 */
    int32_t half_a;             /* angle window, steps, default 360; 0 .. 1024 */
    float angle_step;           /* radians per step, default 0.5 degrees; finite, > 0 */
    int32_t coarse_shift;       /* default 4; 0 .. 5 */
    int32_t max_refine_blocks;  /* default 16384; >= 1 */
} dpg_loc_params;

#define DPG_LOC_OK 0
#define DPG_LOC_NO_OVERLAP 1
#define DPG_LOC_UNPROVEN 2
typedef struct dpg_loc_result {
    float pose[3];              /* x, y, theta in the map frame (the frame of est_poses) */
    float rot[2];               /* (c_a, s_a) of the winner */
    int32_t score;              /* the winner's score */
    int32_t score_at_guess;     /* score(half_a, 0, 0) */
    int32_t n_pts;              /* the largest possible score is 255 n_pts */
    int32_t best_a, best_dx, best_dy;
    int32_t status;             /* DPG_LOC_* */
    int32_t n_seeds;            /* 2 half_a + 1 */
    int32_t box[4];             /* x0, y0, w, h of the field */
    int32_t pad;
    int64_t n_blocks;          /* (2 half_a + 1) nbx nby */
    int64_t n_frontier;
    int64_t n_refined_candidates;   /* in-window candidates scored in steps 3 and 5 (a seed that is
                                       also in the frontier counts twice; an overflowed frontier: step 3 only) */
    double ms_kernels;          /* ms_field + ms_bound + ms_fine */
    double ms_field;            /* grid, threshold-and-stencil and pooling (HIP events) */
    double ms_bound;            /* keys, bounds and seeds */
    double ms_fine;             /* seed scoring, compaction, frontier scoring, reductions */
} dpg_loc_result;

#define DPG_LOC_PARAMS_SIZE 56
#define DPG_LOC_RESULT_SIZE 128
#ifdef __cplusplus
 static_assert(sizeof(dpg_loc_params) == DPG_LOC_PARAMS_SIZE && sizeof(dpg_loc_result) == DPG_LOC_RESULT_SIZE, "loc ABI structs");
#else
 _Static_assert(sizeof(dpg_loc_params) == DPG_LOC_PARAMS_SIZE && sizeof(dpg_loc_result) == DPG_LOC_RESULT_SIZE, "loc ABI structs");
#endif

void dpg_loc_params_default(dpg_loc_params* p);
/* Host.  DPG_OK or DPG_ERR_ARG: every field against the ranges above (resolution 0 is valid). */
int dpg_loc_params_check(const dpg_loc_params* p);
/* Host.  rot_out[2 half_a + 1][2] = (c_a, s_a). */
int dpg_loc_rotations(float guess_theta, const dpg_loc_params* p, float* rot_out);
/* The localisation of cloud_xy[n_pts][2] (body frame) around guess = (x, y, theta); blocks until
 * *result is written (only on success).  Errors: DPG_ERR_ARG -- params, n_pts < 0 or above 2^23, an
 * invalid guess key, NULL arguments, n_nodes out of range; DPG_ERR_STATE -- a multi-device, virtual
 * or rank context; DPG_ERR_SIZE -- the box above max_cells, or a search above the sizes above. */
int dpg_map_localize(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const float* cloud_xy, int64_t n_pts,
                     const float guess[3], const dpg_loc_params* params, dpg_loc_result* result);
/* Diagnostics.  Each: cap in elements of out, DPG_ERR_SIZE with nothing written when too small.
 * dpg_map_field: shift < 0 -- F [h][w]; shift 0 .. 5 -- P at that shift (params' coarse_shift is not
 * read), [h + s - 1][w + s - 1]; box receives x0, y0, w, h (also when out is NULL: plan only). */
int dpg_map_field(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const dpg_loc_params* params, int32_t shift,
                  uint8_t* out, int64_t cap, int32_t box[4]);
/* the bound volume, out[2 half_a + 1][nby][nbx] */
int dpg_map_localize_bounds(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const float* cloud_xy, int64_t n_pts,
                            const float guess[3], const dpg_loc_params* params, int32_t* out, int64_t cap);
/* the exact score volume, out[2 half_a + 1][2 half_y + 1][2 half_x + 1], from the search's own fine
 * kernel run over every block */
int dpg_map_localize_scores(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const float* cloud_xy, int64_t n_pts,
                            const float guess[3], const dpg_loc_params* params, int32_t* out, int64_t cap);

/* ---- frozen map: a kept likelihood field that scans are localised and tracked against ----
 * dpg_map_localize rebuilds grid and field on every call.  A dpg_fmap holds F, its box and its
 * resolution in buffers of its own: it is built (or loaded) once, searched any number of times, and
 * keeps no reference to the store it was taken from -- the store may be appended to, relabelled or
 * destroyed afterwards and the map does not change.  "Frozen" means exactly that: a re-optimised
 * graph, or a map whose nodes changed, needs a new freeze.  A map is a child of its context
 * (dpg_ctx_destroy destroys it), runs on the context's stream and exists on single-device contexts
 * only: the creators return NULL (dpg_last_error) on a multi-device, virtual or rank context, the
 * other calls DPG_ERR_STATE.  The reference has no such stage.
 *
 * dpg_fmap_create: the grid and the field exactly as dpg_map_localize makes them for (d, n_nodes,
 *   est_poses, params) -- box, res and the bytes of dpg_map_field(shift < 0) -- copied into the
 *   handle.  Of params only resolution, max_cells, margin_cells, sigma, kernel_radius and occupied_min
 *   matter (all of it is checked).  No active node gives an empty map (w = h = 0): valid, and every
 *   search on it answers DPG_LOC_NO_OVERLAP.
 * dpg_fmap_from_field: F [h][w] as given (any bytes), box = (x0, y0, w, h); sigma, kernel_radius and
 *   occupied_min only describe how F was made.  DPG_ERR_ARG (NULL): res not finite or <= 0, w or
 *   h < 0, w h above 2^25, F NULL with w h > 0.
 * File (dpg_fmap_save / _load), little-endian: a 64-byte header, then F row-major.
 *     0 magic "DPGFMAP1" | 8 uint32 version = 1 | 12 int32 kernel_radius | 16 int32 occupied_min |
 *    20 float sigma | 24 double res | 32 int32 box[4] | 48 int64 n_bytes = w h | 56 eight zero bytes
 *   dpg_fmap_header_check (host, plain C): DPG_OK, or DPG_ERR_ARG for a wrong magic or version, a
 *   bad box or res (as dpg_fmap_from_field), n_bytes != w h, file_bytes != 64 + n_bytes, or a
 *   non-zero reserved byte.  dpg_fmap_load returns NULL for such a file or one it cannot read. */
typedef struct dpg_fmap dpg_fmap;
typedef struct dpg_fmap_info {
    int32_t box[4];             /* x0, y0, w, h */
    double res;
    float sigma;
    int32_t kernel_radius, occupied_min;
    int32_t pad;
    int64_t n_bytes;            /* w h: the bytes of F held */
} dpg_fmap_info;
#define DPG_FMAP_INFO_SIZE 48
#define DPG_FMAP_HEADER_SIZE 64

dpg_fmap* dpg_fmap_create(dpg_dpg* d, int64_t n_nodes, const float* est_poses, const dpg_loc_params* params);
dpg_fmap* dpg_fmap_from_field(dpg_ctx* ctx, const uint8_t* F, const int32_t box[4], double res, float sigma,
                              int32_t kernel_radius, int32_t occupied_min);
int dpg_fmap_info_get(const dpg_fmap* m, dpg_fmap_info* out);
/* out[h][w] = F; cap in bytes, DPG_ERR_SIZE with nothing written when too small */
int dpg_fmap_fetch(dpg_fmap* m, uint8_t* out, int64_t cap);
void dpg_fmap_destroy(dpg_fmap* m);
int dpg_fmap_save(dpg_fmap* m, const char* path);
dpg_fmap* dpg_fmap_load(dpg_ctx* ctx, const char* path);
int dpg_fmap_header_check(const void* hdr64, int64_t file_bytes);
/* dpg_map_localize's contract word for word, with F, the box and res taken from the map.  Of params,
 * resolution, max_cells, margin_cells, sigma, kernel_radius and occupied_min are NOT read (nor
 * checked).  P for a coarse_shift is pooled from the map's F at the first request for that shift and
 * kept.  ms_field is 0 when the call built nothing (it covers the pooling when it did).  Errors:
 * DPG_ERR_ARG, DPG_ERR_SIZE as dpg_map_localize for the request; DPG_ERR_STATE as above. */
int dpg_fmap_localize(dpg_fmap* m, const float* cloud_xy, int64_t n_pts, const float guess[3],
                      const dpg_loc_params* params, dpg_loc_result* result);

/* dpg_fmap_track: a batch of scans, each searched EXHAUSTIVELY over a small window around its own
 * guess, in one enqueue.  Scan b is clouds_xy[offsets[b] .. offsets[b + 1]); its record is that of
 * dpg_loc_params / dpg_loc_result for the same half_x, half_y, half_a, angle_step and guess at
 * coarse_shift 0: rotations (dpg_loc_rotations' rule), keys, score, the winner and its tie order,
 * pose, rot and score_at_guess.  status: DPG_LOC_NO_OVERLAP when the winner's score is 0, else
 * DPG_LOC_OK.  After the one float transform per point and angle everything is integer: outputs are
 * exact and two calls give the same bytes.  One upload, the launches, one copy back and one
 * synchronisation per call, whatever B is; B = 0 and an empty map launch nothing.
 * Errors, all before anything is launched or written: DPG_ERR_ARG -- NULL arguments, params out of
 * range, B < 0, offsets[0] < 0 or offsets not monotone, a guess whose x or y has no valid key or whose
 * angle is not finite; DPG_ERR_SIZE -- B above 65535, a scan above 2^23 points, more than 2^26
 * points in all; DPG_ERR_STATE as above. */
typedef struct dpg_track_params {
    int32_t half_x, half_y;     /* translation window, cells, default 10, 10; 0 .. 64 */
    int32_t half_a;             /* angle window, steps, default 10; 0 .. 64 */
    float angle_step;           /* radians per step, default 0.5 degrees; finite, > 0 */
} dpg_track_params;
typedef struct dpg_track_result {
    float pose[3];              /* x, y, theta in the map's frame */
    float rot[2];               /* (c_a, s_a) of the winner */
    int32_t score;
    int32_t score_at_guess;     /* score(half_a, 0, 0) */
    int32_t n_pts;              /* the scan's points: the largest possible score is 255 n_pts */
    int32_t best_a, best_dx, best_dy;
    int32_t status;             /* DPG_LOC_OK or DPG_LOC_NO_OVERLAP */
} dpg_track_result;
#define DPG_TRACK_PARAMS_SIZE 16
#define DPG_TRACK_RESULT_SIZE 48
#ifdef __cplusplus
 static_assert(sizeof(dpg_track_params) == DPG_TRACK_PARAMS_SIZE && sizeof(dpg_track_result) == DPG_TRACK_RESULT_SIZE &&
               sizeof(dpg_fmap_info) == DPG_FMAP_INFO_SIZE, "track ABI structs");
#else
 _Static_assert(sizeof(dpg_track_params) == DPG_TRACK_PARAMS_SIZE && sizeof(dpg_track_result) == DPG_TRACK_RESULT_SIZE &&
                sizeof(dpg_fmap_info) == DPG_FMAP_INFO_SIZE, "track ABI structs");
#endif
void dpg_track_params_default(dpg_track_params* p);
/* Host.  DPG_OK or DPG_ERR_ARG: every field against the ranges above. */
int dpg_track_params_check(const dpg_track_params* p);
int dpg_fmap_track(dpg_fmap* m, const float* clouds_xy, const int64_t* offsets, int64_t B, const float* guesses,
                   const dpg_track_params* params, dpg_track_result* out);
/* ms of the two launches of the last dpg_fmap_track that launched anything (HIP events) */
float dpg_fmap_track_kernel_ms(const dpg_fmap* m);

/* dpg_fmap_refine: sub-cell pose refinement of a batch of scans on the map's interpolated field -- a
 * few damped Gauss-Newton steps per scan from a start such as a tracked pose, on the device for the
 * whole batch, with the curvature matrix of the answer.  It reads only F, the box and res, so it
 * works on a loaded map.  The reference has no such stage.  This comment is the contract: the kernel
 * (csrc/dpg_refine.hip) and the numpy restatement (tests/refine_ref.py) are written from it and share
 * no code.  Every fp64 expression below is one rounding per operation (no contraction, no fast-math);
 * the device uses no transcendental and no square root.  Parentheses fix the order.
 *
 * Map.  F uint8 [h][w], box (x0, y0, w, h) and res are the handle's.  Outside the box F reads 0.  An
 *   empty map is not special: every sample reads 0.
 * Start of scan b.  starts[b][5] floats (x, y, theta, c, s): the first five floats of a
 *   dpg_track_result (pose, rot); theta is not read.
 *     ires = 1.0 / res
 *     tu = ((double)x ires) - (double)x0        tv = ((double)y ires) - (double)y0
 *     c = (double)starts[3]   s = (double)starts[4]          (not normalised)
 *   DPG_ERR_ARG when x, y, c or s is not finite, when |(double)x ires| >= 2^29 (or y), or when
 *   (c c) + (s s) is outside [0.5, 2].
 *   dpg_refine_start (host): out = (x, y, theta, (float)cos((double)theta), (float)sin((double)theta)),
 *   dpg_loc_rotations' rule.
 * Evaluation at state (tu, tv, c, s).  Point i is float (x, y); it is used iff both coordinates are
 *   finite and |u|, |v| < 2^29; an unused point adds nothing.
 *     px = (double)x ires            py = (double)y ires
 *     rx = (c px) - (s py)           ry = (s px) + (c py)
 *     u = rx + tu                    v = ry + tv
 *     iu = floor(u), fu = u - iu     iv = floor(v), fv = v - iv     au = 1 - fu, av = 1 - fv
 *     F00 = F[iv][iu]  F10 = F[iv][iu+1]  F01 = F[iv+1][iu]  F11 = F[iv+1][iu+1]      (as doubles)
 *     M  = (av ((au F00) + (fu F10))) + (fv ((au F01) + (fu F11)))
 *     gu = (av (F10 - F00)) + (fv (F11 - F01))
 *     gv = (au (F01 - F00)) + (fu (F11 - F10))
 *     r  = 255 - M                   jt = (gv rx) - (gu ry)
 *   Eleven sums S: gu gu, gu gv, gu jt, gv gv, gv jt, jt jt (H00 H01 H02 H11 H12 H22: the upper
 *   triangle, in cells and radians), gu r, gv r, jt r (b0 b1 b2), r r (cost), r.  n_used is an integer
 *   count beside them.
 * Summation order, 256 lanes.  Lane t adds its points i = t, t + 256, ... in ascending order, each sum
 *   from +0.0.  Within each group of 64 lanes, for stride 32, 16, 8, 4, 2, 1: p[l] += p[l + stride]
 *   for l < stride.  The total is (W0 + W1) + (W2 + W3) over the four groups' lane-0 values.
 * Step from S, with params' lambda, max_step_cells, max_step_angle, tol_cells, tol_angle and
 *   eps = 1e-12:
 *     D1 = H11 + (lambda H11)          D2 = H22 + (lambda H22)
 *     d0 = H00 + (lambda H00)                                   pivot: d0 > 0
 *     l10 = H01/d0    l20 = H02/d0
 *     d1 = D1 - (l10 H01)                                       pivot: d1 > eps D1
 *     e12 = H12 - (l20 H01)            l21 = e12/d1
 *     d2 = (D2 - (l20 H02)) - (l21 e12)                         pivot: d2 > eps D2
 *     y0 = b0    y1 = b1 - (l10 y0)    y2 = (b2 - (l20 y0)) - (l21 y1)
 *     z2 = y2/d2    z1 = (y1/d1) - (l21 z2)    z0 = ((y0/d0) - (l10 z1)) - (l20 z2)
 *   A failed pivot or a non-finite z: DEGENERATE.  du, dv = z0, z1 clamped to +-max_step_cells,
 *   dt = z2 clamped to +-max_step_angle.  Converged when |du| < tol_cells and |dv| < tol_cells and
 *   |dt| < tol_angle; the step is then not applied.  Apply: tu += du; tv += dv; a = dt 0.5; q = a a;
 *   den = 1 + q; cd = (1 - q)/den; sd = (a + a)/den; (c, s) <- ((c cd) - (s sd), (s cd) + (c sd)) -- the
 *   Cayley form, an exact rotation without trigonometry.
 * Loop, for k = 0 .. max_iters: 1. evaluate at iterate k; 2. if k == 0 or cost_k < best.cost (strict:
 *   the earlier iterate wins a tie), best = (k, state, S, n_used); 3. n_used == 0 at k = 0 stops with
 *   NO_POINTS; 4. k == max_iters stops with MAX_ITERS; 5. otherwise the step, which may stop with
 *   DEGENERATE or CONVERGED.  The answer is `best`: a refinement never returns a worse cost than its
 *   start.  n_evals is the number of evaluations made.
 * Record (host, plain C): pose x = (float)((tu + (double)x0) res), y alike; theta =
 *   dpg_refine_angle(c, s) = (float)atan2(s, c); rot = ((float)c, (float)s); cost = S[9], sum_r = S[10]
 *   and hess = S[0..5] of the best iterate, undamped; cost_start = the cost of evaluation 0.
 *   cov = s2 H^-1 in metres and radians: s2 = cost / (double)max(n_used - 3, 1); column j of H^-1 is
 *   the z of the step's expressions at lambda = 0 for b = the unit vector e_j, and entry (i, j), i <= j,
 *   is taken from column j; cov = ((s2 h00) (res res), (s2 h01) (res res), (s2 h02) res,
 *   (s2 h11) (res res), (s2 h12) res, s2 h22).  A failed pivot or a non-finite entry: cov_ok = 0 and
 *   zeros.  cov is the least-squares curvature estimate in the field's own residual units (bytes of
 *   F), not a calibrated sensor model: it ranks directions and scans, it is not a metric variance.
 * Calls.  Single-device contexts only (DPG_ERR_STATE).  Every error is raised before anything is
 *   launched or written.  B = 0 launches nothing.  One upload, one copy back and one synchronisation
 *   per call, whatever B is.  Limits as dpg_fmap_track: B <= 65535, a scan <= 2^23 points, <= 2^26
 *   points in all (DPG_ERR_SIZE); DPG_ERR_ARG for NULL arguments, B < 0, bad offsets, parameters out
 *   of range, or a start as above.  Two calls give the same bytes. */
typedef struct dpg_refine_params {
    int32_t max_iters;          /* steps at most, default 20; 0 .. 64 */
    int32_t pad;
    double lambda;              /* Levenberg damping of the diagonal, default 1e-3; finite, >= 0 */
    double max_step_cells;      /* default 1.0; > 0 */
    double max_step_angle;      /* radians, default 0.02; > 0 */
    double tol_cells;           /* default 1e-3; >= 0 */
    double tol_angle;           /* default 1e-5; >= 0 */
} dpg_refine_params;
#define DPG_REFINE_CONVERGED 0
#define DPG_REFINE_MAX_ITERS 1
#define DPG_REFINE_DEGENERATE 2
#define DPG_REFINE_NO_POINTS 3
typedef struct dpg_refine_result {
    float pose[3];              /* x, y, theta of the best iterate, in the map's frame */
    float rot[2];               /* ((float)c, (float)s) */
    int32_t status;             /* DPG_REFINE_* */
    int32_t n_evals;            /* evaluations made, 1 .. max_iters + 1 */
    int32_t best_eval;          /* the evaluation the answer is from */
    int32_t n_used;             /* points used by that evaluation */
    int32_t pad;
    double tu, tv, c, s;        /* the best iterate's state, in cells */
    double cost, cost_start;    /* sum of r r at the best iterate and at evaluation 0 */
    double sum_r;
    double hess[6];             /* H00 H01 H02 H11 H12 H22, cells and radians, undamped */
    double cov[6];              /* xx xy xt yy yt tt, metres and radians (see above) */
    int32_t cov_ok;
    int32_t pad2;
} dpg_refine_result;
#define DPG_REFINE_PARAMS_SIZE 48
#define DPG_REFINE_RESULT_SIZE 200
#define DPG_REFINE_TRACE_COLS 16
#ifdef __cplusplus
 static_assert(sizeof(dpg_refine_params) == DPG_REFINE_PARAMS_SIZE && sizeof(dpg_refine_result) == DPG_REFINE_RESULT_SIZE,
               "refine ABI structs");
#else
 _Static_assert(sizeof(dpg_refine_params) == DPG_REFINE_PARAMS_SIZE && sizeof(dpg_refine_result) == DPG_REFINE_RESULT_SIZE,
                "refine ABI structs");
#endif
void dpg_refine_params_default(dpg_refine_params* p);
/* Host.  DPG_OK or DPG_ERR_ARG: every field against the ranges above (NaN and inf are out of range). */
int dpg_refine_params_check(const dpg_refine_params* p);
/* Host.  The start of a pose: out = (x, y, theta, (float)cos((double)theta), (float)sin((double)theta)). */
int dpg_refine_start(const float pose[3], float out[5]);
/* Host.  (float)atan2(s, c): the record's theta. */
float dpg_refine_angle(double c, double s);
int dpg_fmap_refine(dpg_fmap* m, const float* clouds_xy, const int64_t* offsets, int64_t B, const float* starts,
                    const dpg_refine_params* params, dpg_refine_result* out);
/* dpg_fmap_refine with a diagnostic output: trace[B][max_iters + 1][16] doubles, per evaluation
 * tu, tv, c, s, the eleven sums and n_used as a double; rows past n_evals are zero.  cap in doubles:
 * DPG_ERR_SIZE with nothing written when it is below B (max_iters + 1) 16. */
int dpg_fmap_refine_trace(dpg_fmap* m, const float* clouds_xy, const int64_t* offsets, int64_t B, const float* starts,
                          const dpg_refine_params* params, dpg_refine_result* out, double* trace, int64_t cap);
/* dpg_fmap_track and the refinement of its winners, enqueued back to back with no host
 * synchronisation in between: the start of scan b is derived on the device from its track record by
 * the expressions above (x = (float)((double)(cx + best_dx) res), y alike, (c, s) = the winner's rot).
 * track_out is byte for byte dpg_fmap_track's, refine_out byte for byte dpg_fmap_refine's of
 * track_out.  A scan whose track status is DPG_LOC_NO_OVERLAP is refined all the same: the caller
 * decides what to do with it.  Errors as the two calls; a guess so far out that some shift of its
 * window would make a start beyond 2^29 cells is DPG_ERR_ARG. */
int dpg_fmap_track_refine(dpg_fmap* m, const float* clouds_xy, const int64_t* offsets, int64_t B, const float* guesses,
                          const dpg_track_params* track_params, const dpg_refine_params* refine_params,
                          dpg_track_result* track_out, dpg_refine_result* refine_out);
/* ms of the refinement launch of the last call that launched one (HIP events) */
float dpg_fmap_refine_kernel_ms(const dpg_fmap* m);

#ifdef __cplusplus
}
#endif
#endif /* DPG_SLAM_C_H */
