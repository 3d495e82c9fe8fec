/*
 * dpg_host.c -- host-side data path of the DPG-SLAM hot path (no GPU work here).
 *
 * R1 polar scan -> base_link cloud: MeasurementPoint ctor (src/dpg_slam/dpg_measurement.h:41-46),
 *    getPointInLaserFrame (:102-104), createNode (src/dpg_slam/dpg_slam.cc:488-513),
 *    DpgNode::getCachedPointCloudFromNode (src/dpg_slam/dpg_node.cc:8-25).
 * R2 downsamplePointCloud (dpg_slam.cc:346-360).
 * R3 runIcp initial guess (dpg_slam.cc:364-378) via math_utils::inverseTransformPoint
 *    (src/dpg_slam/math_utils.cc:21-35).
 * R9 odometry factor noise (dpg_slam.cc:53-75, 216-238).
 *
 * These run on the host in float exactly as the reference evaluates them, so the clouds the GPU
 * receives are bit-identical to what the CPU path would build.  Built with -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dpg_slam_c.h"
#include "dpg_internal.h"

/* math_utils::AngleMod<float> (math_utils.h:13-16): float in, the subtraction runs in double. */
static float angle_mod(float a) {
    double v = (double)a;
    v -= (M_PI * 2.0) * rint(v / (M_PI * 2.0));
    return (float)v;
}

/* Eigen::Rotation2Df(theta) * (x, y): [cos -sin; sin cos] times the vector, float. */
static void rotate(float theta, float x, float y, float* ox, float* oy) {
    const float c = cosf(theta), s = sinf(theta);
    const float ms = -s;
    *ox = c * x + ms * y;
    *oy = s * x + c * y;
}

int64_t dpg_scan_to_cloud(const float* ranges, int64_t n_ranges, float angle_min, float angle_max,
                          float range_max, float laser_x, float laser_y, float laser_theta,
                          float* xy_out) {
    if (!ranges || !xy_out || n_ranges <= 0) return 0;
    /* dpg_slam.cc:497 -- (float - float) / (size - 1.0) in double, stored as float */
    const float angle_inc = (float)((double)(angle_max - angle_min) / ((double)n_ranges - 1.0));
    int64_t n = 0;
    for (int64_t i = 0; i < n_ranges; ++i) {
        const float r = ranges[i];
        if (r >= range_max) continue; /* label MAX_RANGE, skipped by the cloud cache */
        const float angle = angle_inc * (float)i + angle_min;
        const float lx = r * cosf(angle), ly = r * sinf(angle);
        float bx, by;
        rotate(laser_theta, lx, ly, &bx, &by);
        xy_out[2 * n] = laser_x + bx;
        xy_out[2 * n + 1] = laser_y + by;
        ++n;
    }
    return n;
}

int64_t dpg_downsample_cloud(const float* xy, int64_t n, int32_t ratio, float* xy_out) {
    if (!xy || !xy_out || n <= 0) return 0;
    if (ratio < 1) ratio = 1;
    int64_t k = 0;
    for (int64_t i = 0; i < n; i += ratio, ++k) {
        xy_out[2 * k] = xy[2 * i];
        xy_out[2 * k + 1] = xy[2 * i + 1];
    }
    return k;
}

void dpg_inverse_transform_point(const float a[3], const float b[3], float out[3]) {
    const float dx = a[0] - b[0], dy = a[1] - b[1];
    rotate(-b[2], dx, dy, &out[0], &out[1]);
    out[2] = angle_mod(a[2] - b[2]);
}

void dpg_transform_point(const float p[3], const float frame[3], float out[3]) {
    float rx, ry;
    rotate(frame[2], p[0], p[1], &rx, &ry);
    out[0] = frame[0] + rx;
    out[1] = frame[1] + ry;
    out[2] = angle_mod(frame[2] + p[2]);
}

void dpg_icp_guess(const float pose_src[3], const float pose_tgt[3], float g[6]) {
    float d[3];
    dpg_inverse_transform_point(pose_src, pose_tgt, d);
    const float c = cosf(d[2]), s = sinf(d[2]);
    g[0] = c;
    g[1] = -s;
    g[2] = d[0];
    g[3] = s;
    g[4] = c;
    g[5] = d[1];
}

void dpg_icp_params_default(dpg_icp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->icp_maximum_iterations = 500;             /* parameters.h:146 */
    p->icp_use_reciprocal_correspondences = 1;   /* parameters.h:201 */
    p->icp_maximum_transformation_epsilon = 0.000000005; /* parameters.h:159 */
    p->icp_max_correspondence_distance = 0.6;    /* parameters.h:173 */
    p->ransac_iterations = 50;                   /* parameters.h:191 */
    p->downsample_icp_points_ratio = 5;          /* parameters.h:402 */
    p->laser_x_variance = 0.5f;                  /* parameters.h:374 */
    p->laser_y_variance = 0.5f;                  /* parameters.h:385 */
    p->laser_theta_variance = 0.3f;              /* parameters.h:396 */
    p->min_number_correspondences = 3;           /* pcl::Registration default */
    p->mse_threshold_absolute = 1e-12;           /* pcl DefaultConvergenceCriteria default */
}

void dpg_gn_params_default(dpg_gn_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 100;
    p->use_error_criteria = 0;
    p->delta_tol = 1e-10;
    p->relative_error_tol = 1e-5;
    p->absolute_error_tol = 1e-5;
    p->pcg_rel_tol = 1e-12;
    p->pcg_max_iterations = 20000;
    p->pcg_check_every = 16;
    p->reuse_factorization = 1;
    p->refactor_delta = 1e-3;
}

void dpg_grid_params_default(dpg_grid_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->margin_cells = 1;
}

/* occupancy byte of a cell: unknown (-1) without an observation, else 100 hits / n rounded half up */
void dpg_occupancy_from_counts(const int32_t* hits, const int32_t* misses, int64_t n, int8_t* occ) {
    for (int64_t c = 0; c < n; ++c) {
        const int64_t h = hits[c], t = h + (int64_t)misses[c];
        occ[c] = t == 0 ? (int8_t)-1 : (int8_t)((200 * h + t) / (2 * t));
    }
}

/* the grid's box: every ray of an active node stays within the node's largest range of its lidar */
int dpg_grid_box(const float* lidar_xy, const float* r_v, const uint8_t* active, int64_t n, double res,
                 int32_t margin, int32_t box[4]) {
    if (!box || n < 0 || (n > 0 && (!lidar_xy || !r_v)) || !(res > 0.0) || !isfinite(res) || margin < 0)
        return DPG_ERR_ARG;
    double xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
    int any = 0;
    for (int64_t v = 0; v < n; ++v) {
        if (active && !active[v]) continue;
        const double x = (double)lidar_xy[2 * v], y = (double)lidar_xy[2 * v + 1], r = (double)r_v[v];
        if (!isfinite(x) || !isfinite(y) || !isfinite(r)) return DPG_ERR_ARG;
        any = 1;
        xlo = fmin(xlo, x - r); xhi = fmax(xhi, x + r);
        ylo = fmin(ylo, y - r); yhi = fmax(yhi, y + r);
    }
    box[0] = box[1] = box[2] = box[3] = 0;
    if (!any) return DPG_OK;
    const double lim = 536870912.0; /* 2^29: keys and sides stay inside int32 */
    const double x0 = floor(xlo / res) - margin, x1 = ceil(xhi / res) + margin;
    const double y0 = floor(ylo / res) - margin, y1 = ceil(yhi / res) + margin;
    if (x0 < -lim || y0 < -lim || x1 > lim || y1 > lim) return DPG_ERR_SIZE;
    box[0] = (int32_t)x0;
    box[1] = (int32_t)y0;
    box[2] = (int32_t)(x1 - x0 + 1.0);
    box[3] = (int32_t)(y1 - y0 + 1.0);
    return DPG_OK;
}

/* ---- correlative scan matching: parameters, smoothing table, rotations (the contract is in
 * include/dpg_slam_c.h) ---- */
void dpg_csm_params_default(dpg_csm_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->resolution = 0.1f;
    p->sigma = 0.1f;
    p->kernel_radius = 3;
    p->half_cells = 160;
    p->half_x = 15;
    p->half_y = 15;
    p->half_a = 20;
    p->angle_step = (float)(0.5 * M_PI / 180.0);
}

int64_t dpg_csm_lds_bytes(const dpg_csm_params* p) {
    if (!p) return DPG_ERR_ARG;
    if (!(p->resolution > 0.0f) || !isfinite(p->resolution) || !(p->sigma > 0.0f) || !isfinite(p->sigma) ||
        !(p->angle_step > 0.0f) || !isfinite(p->angle_step))
        return DPG_ERR_ARG;
    if (p->kernel_radius < 0 || p->kernel_radius > 7 || p->half_cells < 0 || p->half_x < 0 || p->half_x > 64 ||
        p->half_y < 0 || p->half_y > 64 || p->half_a < 0 || p->half_a > 64)
        return DPG_ERR_ARG;
    if (p->half_cells > DPG_CSM_LDS_BUDGET) return DPG_ERR_ARG;   /* the product below stays in int64 */
    const int64_t w = 2 * (int64_t)p->half_cells + 1 + 4 * (int64_t)p->half_x;
    const int64_t h = 2 * (int64_t)p->half_cells + 1 + 4 * (int64_t)p->half_y;
    const int64_t bytes = (w * h + 15) / 16 * 16 + DPG_CSM_LDS_FIXED;
    return bytes <= DPG_CSM_LDS_BUDGET ? bytes : DPG_ERR_ARG;
}

int dpg_csm_lut(const dpg_csm_params* p, uint8_t* lut_out) {
    if (!lut_out || dpg_csm_lds_bytes(p) < 0) return DPG_ERR_ARG;
    const double res = (double)p->resolution, sigma = (double)p->sigma;
    const int n = p->kernel_radius * p->kernel_radius;
    for (int d2 = 0; d2 <= n; ++d2)
        lut_out[d2] = (uint8_t)floor(255.0 * exp(-(double)d2 * res * res / (2.0 * sigma * sigma)) + 0.5);
    return DPG_OK;
}

int dpg_csm_rotations(const float guess[6], const dpg_csm_params* p, float* rot_out) {
    if (!guess || !rot_out || dpg_csm_lds_bytes(p) < 0) return DPG_ERR_ARG;
    const double tg = atan2((double)guess[3], (double)guess[0]);
    for (int a = 0; a <= 2 * p->half_a; ++a) {
        const double ang = tg + (double)(a - p->half_a) * (double)p->angle_step;
        rot_out[2 * a] = (float)cos(ang);
        rot_out[2 * a + 1] = (float)sin(ang);
    }
    return DPG_OK;
}

/* ---- loop-closure verification: parameters, sensor key, LDS bytes (the contract is in
 * include/dpg_slam_c.h) ---- */
void dpg_verify_params_default(dpg_verify_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->resolution = 0.1f;
    p->half_cells = 160;
    p->occ_radius = 2;
    p->sensor[0] = 0.2f;
    p->sensor[1] = 0.0f;
}

int dpg_verify_sensor_key(const dpg_verify_params* p, int32_t key[2]) {
    if (!p || !key || !(p->resolution > 0.0f) || !isfinite(p->resolution)) return DPG_ERR_ARG;
    for (int k = 0; k < 2; ++k) {
        const double q = (double)p->sensor[k] / (double)p->resolution;
        if (!(fabs(q) < 536870912.0)) return DPG_ERR_ARG;   /* non-finite too */
        key[k] = (int32_t)round(q);
    }
    return DPG_OK;
}

int dpg_verify_params_check(const dpg_verify_params* p) {
    int32_t a[2];
    if (dpg_verify_sensor_key(p, a)) return DPG_ERR_ARG;
    if (p->half_cells < 0 || p->occ_radius < 0 || p->occ_radius > 7) return DPG_ERR_ARG;
    if (abs(a[0]) > p->half_cells || abs(a[1]) > p->half_cells) return DPG_ERR_ARG;
    return DPG_OK;
}

int64_t dpg_verify_lds_bytes(const dpg_verify_params* p) {
    if (dpg_verify_params_check(p)) return DPG_ERR_ARG;
    if (p->half_cells > DPG_VERIFY_LDS_BUDGET) return DPG_ERR_ARG;   /* the product below stays in int64 */
    const int64_t w = 2 * (int64_t)p->half_cells + 1;
    const int64_t plane = ((w * w + 31) / 32 * 4 + 15) / 16 * 16;
    const int64_t bytes = 2 * plane + DPG_VERIFY_LDS_FIXED;
    return bytes <= DPG_VERIFY_LDS_BUDGET ? bytes : DPG_ERR_ARG;
}

/* ---- localisation in the active map: parameters and rotations (the contract is in
 * include/dpg_slam_c.h) ---- */
void dpg_loc_params_default(dpg_loc_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->margin_cells = 1;
    p->sigma = 0.1f;
    p->kernel_radius = 3;
    p->occupied_min = 50;
    p->half_x = 40;
    p->half_y = 40;
    p->half_a = 360;
    p->angle_step = (float)(0.5 * M_PI / 180.0);
    p->coarse_shift = 4;
    p->max_refine_blocks = 16384;
}

int dpg_loc_params_check(const dpg_loc_params* p) {
    if (!p) return DPG_ERR_ARG;
    if (!(p->resolution >= 0.0) || !isfinite(p->resolution) || !(p->sigma > 0.0f) || !isfinite(p->sigma) ||
        !(p->angle_step > 0.0f) || !isfinite(p->angle_step))
        return DPG_ERR_ARG;
    if (p->max_cells < 0 || p->max_cells > (int64_t)1 << 25 || p->margin_cells < 0) return DPG_ERR_ARG;
    if (p->kernel_radius < 0 || p->kernel_radius > 7 || p->occupied_min < 1 || p->occupied_min > 100) return DPG_ERR_ARG;
    if (p->half_x < 0 || p->half_x > 32768 || p->half_y < 0 || p->half_y > 32768 || p->half_a < 0 || p->half_a > 1024)
        return DPG_ERR_ARG;
    if (p->coarse_shift < 0 || p->coarse_shift > 5 || p->max_refine_blocks < 1) return DPG_ERR_ARG;
    return DPG_OK;
}

int dpg_loc_rotations(float guess_theta, const dpg_loc_params* p, float* rot_out) {
    if (!rot_out || dpg_loc_params_check(p)) return DPG_ERR_ARG;
    for (int a = 0; a <= 2 * p->half_a; ++a) {
        const double ang = (double)guess_theta + (double)(a - p->half_a) * (double)p->angle_step;
        rot_out[2 * a] = (float)cos(ang);
        rot_out[2 * a + 1] = (float)sin(ang);
    }
    return DPG_OK;
}

void dpg_track_params_default(dpg_track_params* p) {
    if (!p) return;
    p->half_x = 10;
    p->half_y = 10;
    p->half_a = 10;
    p->angle_step = (float)(0.5 * M_PI / 180.0);
}

int dpg_track_params_check(const dpg_track_params* p) {
    if (!p) return DPG_ERR_ARG;
    if (p->half_x < 0 || p->half_x > 64 || p->half_y < 0 || p->half_y > 64 || p->half_a < 0 || p->half_a > 64) return DPG_ERR_ARG;
    if (!(p->angle_step > 0.0f) || !isfinite(p->angle_step)) return DPG_ERR_ARG;
    return DPG_OK;
}

/* ---- dpg_fmap_refine: parameters, starts and the record (the contract is above dpg_refine_params in
 * include/dpg_slam_c.h; every expression stands as written there) ---- */
void dpg_refine_params_default(dpg_refine_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iters = 20;
    p->lambda = 1e-3;
    p->max_step_cells = 1.0;
    p->max_step_angle = 0.02;
    p->tol_cells = 1e-3;
    p->tol_angle = 1e-5;
}

int dpg_refine_params_check(const dpg_refine_params* p) {
    if (!p) return DPG_ERR_ARG;
    if (p->max_iters < 0 || p->max_iters > 64) return DPG_ERR_ARG;
    if (!(p->lambda >= 0.0) || !isfinite(p->lambda)) return DPG_ERR_ARG;
    if (!(p->max_step_cells > 0.0) || !isfinite(p->max_step_cells) || !(p->max_step_angle > 0.0) || !isfinite(p->max_step_angle))
        return DPG_ERR_ARG;
    if (!(p->tol_cells >= 0.0) || !isfinite(p->tol_cells) || !(p->tol_angle >= 0.0) || !isfinite(p->tol_angle)) return DPG_ERR_ARG;
    return DPG_OK;
}

int dpg_refine_start(const float pose[3], float out[5]) {
    if (!pose || !out) return DPG_ERR_ARG;
    out[0] = pose[0];
    out[1] = pose[1];
    out[2] = pose[2];
    out[3] = (float)cos((double)pose[2]);
    out[4] = (float)sin((double)pose[2]);
    return DPG_OK;
}

float dpg_refine_angle(double c, double s) { return (float)atan2(s, c); }

int dpg_refine_start_check(const float start[5], double ires) {
    const double c = (double)start[3], s = (double)start[4];
    if (!isfinite(start[0]) || !isfinite(start[1]) || !isfinite(start[3]) || !isfinite(start[4])) return DPG_ERR_ARG;
    if (!(fabs((double)start[0] * ires) < 536870912.0) || !(fabs((double)start[1] * ires) < 536870912.0)) return DPG_ERR_ARG;
    const double n2 = (c * c) + (s * s);
    if (!(n2 >= 0.5 && n2 <= 2.0)) return DPG_ERR_ARG;
    return DPG_OK;
}

/* the step's solve: H = (H00 H01 H02 H11 H12 H22), z = (H + lambda diag H)^-1 b; 0 for a failed pivot */
static int refine_solve(const double H[6], double lambda, const double b[3], double z[3]) {
    const double eps = 1e-12;
    const double D1 = H[3] + (lambda * H[3]), D2 = H[5] + (lambda * H[5]);
    const double d0 = H[0] + (lambda * H[0]);
    if (!(d0 > 0.0)) return 0;
    const double l10 = H[1] / d0, l20 = H[2] / d0;
    const double d1 = D1 - (l10 * H[1]);
    if (!(d1 > eps * D1)) return 0;
    const double e12 = H[4] - (l20 * H[1]), l21 = e12 / d1;
    const double d2 = (D2 - (l20 * H[2])) - (l21 * e12);
    if (!(d2 > eps * D2)) return 0;
    const double y0 = b[0], y1 = b[1] - (l10 * y0), y2 = (b[2] - (l20 * y0)) - (l21 * y1);
    z[2] = y2 / d2;
    z[1] = (y1 / d1) - (l21 * z[2]);
    z[0] = ((y0 / d0) - (l10 * z[1])) - (l20 * z[2]);
    return 1;
}

void dpg_refine_record(int32_t status, int32_t n_evals, int32_t best_eval, int32_t n_used, const double state[4],
                       const double S[11], double cost_start, const int32_t box[4], double res, dpg_refine_result* out) {
    dpg_refine_result r;
    memset(&r, 0, sizeof(r));
    r.pose[0] = (float)((state[0] + (double)box[0]) * res);
    r.pose[1] = (float)((state[1] + (double)box[1]) * res);
    r.pose[2] = dpg_refine_angle(state[2], state[3]);
    r.rot[0] = (float)state[2];
    r.rot[1] = (float)state[3];
    r.status = status;
    r.n_evals = n_evals;
    r.best_eval = best_eval;
    r.n_used = n_used;
    r.tu = state[0]; r.tv = state[1]; r.c = state[2]; r.s = state[3];
    r.cost = S[9];
    r.cost_start = cost_start;
    r.sum_r = S[10];
    for (int i = 0; i < 6; ++i) r.hess[i] = S[i];
    /* cov = s2 H^-1: column j from the unit vector e_j, entry (i, j), i <= j, from column j */
    const double s2 = S[9] / (double)(n_used - 3 > 1 ? n_used - 3 : 1);
    double col[3][3];
    int ok = 1;
    for (int j = 0; j < 3 && ok; ++j) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        ok = refine_solve(S, 0.0, e, col[j]);
    }
    if (ok) {
        const double rr = res * res;
        r.cov[0] = (s2 * col[0][0]) * rr;
        r.cov[1] = (s2 * col[1][0]) * rr;
        r.cov[2] = (s2 * col[2][0]) * res;
        r.cov[3] = (s2 * col[1][1]) * rr;
        r.cov[4] = (s2 * col[2][1]) * res;
        r.cov[5] = s2 * col[2][2];
        for (int i = 0; i < 6; ++i)
            if (!isfinite(r.cov[i])) ok = 0;
        if (!ok) memset(r.cov, 0, sizeof(r.cov));
    }
    r.cov_ok = ok;
    *out = r;
}

/* the frozen map's file header (the layout is in dpg_slam_c.h); the host is little-endian */
int dpg_fmap_header_check(const void* hdr64, int64_t file_bytes) {
    if (!hdr64) return DPG_ERR_ARG;
    const unsigned char* h = (const unsigned char*)hdr64;
    uint32_t version;
    double res;
    int32_t box[4];
    int64_t n_bytes;
    if (memcmp(h, "DPGFMAP1", 8) != 0) return DPG_ERR_ARG;
    memcpy(&version, h + 8, 4);
    memcpy(&res, h + 24, 8);
    memcpy(box, h + 32, 16);
    memcpy(&n_bytes, h + 48, 8);
    if (version != 1u) return DPG_ERR_ARG;
    if (!(res > 0.0) || !isfinite(res)) return DPG_ERR_ARG;
    if (box[2] < 0 || box[3] < 0 || (int64_t)box[2] * box[3] > (int64_t)1 << 25) return DPG_ERR_ARG;
    if (n_bytes != (int64_t)box[2] * box[3] || file_bytes != DPG_FMAP_HEADER_SIZE + n_bytes) return DPG_ERR_ARG;
    for (int i = 56; i < 64; ++i)
        if (h[i]) return DPG_ERR_ARG;
    return DPG_OK;
}

/* R9: odometry BetweenFactor from two odom_only_estimates (dpg_slam.cc:56-75). */
int dpg_odometry_factor(const float odom_prev[3], const float odom_cur[3], int32_t i_prev, int32_t i_cur,
                        float transl_from_transl, float transl_from_rot, float rot_from_transl,
                        float rot_from_rot, dpg_factor* out) {
    float d[3];
    dpg_inverse_transform_point(odom_cur, odom_prev, d);
    const float norm = sqrtf(d[0] * d[0] + d[1] * d[1]);       /* Vector2f::norm() */
    const float transl_sd = (transl_from_transl * norm) + (transl_from_rot * fabsf(d[2]));
    const float rot_sd = (rot_from_transl * norm) + (rot_from_rot * fabsf(d[2]));
    memset(out, 0, sizeof(*out));
    out->kind = DPG_FACTOR_BETWEEN;
    out->i = i_prev;
    out->j = i_cur;
    out->z[0] = d[0];
    out->z[1] = d[1];
    out->z[2] = d[2];
    const double st = (double)transl_sd, sr = (double)rot_sd;
    if (!(st > 0.0) || !(sr > 0.0)) return DPG_ERR_NUMERIC; /* GTSAM would build a Constrained model */
    out->info[0] = 1.0 / (st * st);
    out->info[1] = 1.0 / (st * st);
    out->info[2] = 1.0 / (sr * sr);
    return DPG_OK;
}

int dpg_odometry_factors(const float* odom, int64_t n_odom, const int32_t* i_prev, const int32_t* i_cur, int64_t n,
                         float transl_from_transl, float transl_from_rot, float rot_from_transl, float rot_from_rot,
                         dpg_factor* out) {
    if (n < 0 || (n > 0 && (!odom || !i_prev || !i_cur || !out))) return DPG_ERR_ARG;
    int rc = DPG_OK;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t a = i_prev[k], b = i_cur[k];
        if (a < 0 || b < 0 || a >= n_odom || b >= n_odom) return DPG_ERR_ARG;
        const int r = dpg_odometry_factor(odom + 3 * (int64_t)a, odom + 3 * (int64_t)b, a, b, transl_from_transl,
                                          transl_from_rot, rot_from_transl, rot_from_rot, out + k);
        if (r && rc == DPG_OK) rc = r;
    }
    return rc;
}

/* R9: ICP BetweenFactor (addObservationConstraint, dpg_slam.cc:331-338); the covariance is the
 * constant diagonal of calculate_ICP_COV, which GTSAM's smart Gaussian::Covariance reduces to a
 * Diagonal model with precisions 1/variance. */
void dpg_icp_factor(const dpg_icp_result* r, int32_t from_node, int32_t to_node, const dpg_icp_params* p,
                    dpg_factor* out) {
    memset(out, 0, sizeof(*out));
    out->kind = DPG_FACTOR_BETWEEN;
    out->i = from_node;
    out->j = to_node;
    out->z[0] = r->z[0];
    out->z[1] = r->z[1];
    out->z[2] = r->z[2];
    out->info[0] = 1.0 / (double)p->laser_x_variance;
    out->info[1] = 1.0 / (double)p->laser_y_variance;
    out->info[2] = 1.0 / (double)p->laser_theta_variance;
}

/* R1 over a whole scan set: ranges[V][n_beams] -> concatenated clouds + offsets[V+1]. */
int64_t dpg_scans_to_clouds(const float* ranges, int64_t n_nodes, int64_t n_beams, float angle_min,
                            float angle_max, float range_max, float laser_x, float laser_y,
                            float laser_theta, float* xy_out, int64_t* offsets_out) {
    if (!ranges || !xy_out || !offsets_out || n_nodes <= 0) return -1;
    int64_t total = 0;
    offsets_out[0] = 0;
    for (int64_t v = 0; v < n_nodes; ++v) {
        total += dpg_scan_to_cloud(ranges + v * n_beams, n_beams, angle_min, angle_max, range_max, laser_x,
                                   laser_y, laser_theta, xy_out + 2 * total);
        offsets_out[v + 1] = total;
    }
    return total;
}

/* Covariance of the relative pose z = X_i^-1 X_j in z's own tangent frame: to first order
 * dz = A_i d_i + d_j with A_i = -Ad(z^-1), the Jacobians of the Between linearization at zero error
 * (BetweenFactor::evaluateError of GTSAM 4.x: H1 = -z^-1.AdjointMap(), H2 = I), so
 *   cov = A_i Sii A_i^T + A_i Sij + (A_i Sij)^T + Sjj.
 * All blocks row-major; the result is exactly symmetric (the upper triangle mirrored). */
void dpg_relative_covariance(const double xi[3], const double xj[3], const double* Sii, const double* Sij,
                             const double* Sjj, double out[9]) {
    const double d = xj[2] - xi[2], c = cos(d), s = sin(d);
    const double cj = cos(xj[2]), sj = sin(xj[2]);
    const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
    const double A[9] = {-c, -s, -sj * dx + cj * dy, s, -c, -cj * dx - sj * dy, 0.0, 0.0, -1.0};
    double AS[9], N[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) {
            double u = 0.0, v = 0.0;
            for (int k = 0; k < 3; ++k) {
                u += A[3 * r + k] * Sii[3 * k + q];
                v += A[3 * r + k] * Sij[3 * k + q];
            }
            AS[3 * r + q] = u;
            N[3 * r + q] = v;
        }
    for (int r = 0; r < 3; ++r)
        for (int q = r; q < 3; ++q) {
            double m = 0.0;
            for (int k = 0; k < 3; ++k) m += AS[3 * r + k] * A[3 * q + k];
            out[3 * r + q] = out[3 * q + r] = m + (N[3 * r + q] + N[3 * q + r]) + 0.5 * (Sjj[3 * r + q] + Sjj[3 * q + r]);
        }
}

void dpg_relative_triples(const int32_t* pairs, int64_t n, int32_t* tri) {
    for (int64_t q = 0; q < n; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        int32_t* t = tri + 6 * q;
        t[0] = t[1] = t[2] = i;
        t[3] = t[4] = t[5] = j;
    }
}

void dpg_relative_from_blocks(const int32_t* pairs, int64_t n, const double* X, const double* blocks, double* out) {
    for (int64_t q = 0; q < n; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        const double* B = blocks + 27 * q;
        if (i == j) memset(out + 9 * q, 0, 9 * sizeof(double));
        else dpg_relative_covariance(X + 3 * i, X + 3 * j, B, B + 9, B + 18, out + 9 * q);
    }
}

/* Contribution lists per upper block (lin_gather_kernel walks them), in factor order: count, exclusive
 * scan, fill with cptr[u] as block u's cursor -- which leaves every offset one block ahead -- then shift back. */
void dpg_contribution_lists(const dpg_factor* F, int64_t nf, int64_t n, const int32_t* pair, int64_t n_pairs,
                            int32_t* cptr, int32_t* clist) {
    const int64_t nu = n + n_pairs;
    memset(cptr, 0, (size_t)(nu + 1) * sizeof(int32_t));
    for (int64_t k = 0; k < nf; ++k) {
        const int32_t i = F[k].i, j = F[k].j;
        cptr[i]++;
        if (F[k].kind == DPG_FACTOR_BETWEEN) {
            cptr[j]++;
            cptr[n + pair[k]]++;
        }
    }
    int32_t at = 0;   /* (kept in a register: a sum carried through cptr itself is several times slower) */
    for (int64_t u = 0; u <= nu; ++u) { const int32_t c = cptr[u]; cptr[u] = at; at += c; }
    for (int64_t k = 0; k < nf; ++k) {
        const int32_t i = F[k].i, j = F[k].j;
        clist[cptr[i]++] = (int32_t)(k << 2 | 0);
        if (F[k].kind == DPG_FACTOR_BETWEEN) {
            clist[cptr[j]++] = (int32_t)(k << 2 | 1);
            clist[cptr[n + pair[k]]++] = (int32_t)(k << 2 | (i < j ? 2 : 3));
        }
    }
    memmove(cptr + 1, cptr, (size_t)nu * sizeof(int32_t));
    cptr[0] = 0;
}

static void sym6(double* m, int i, int j, double v) { m[6 * i + j] = v; m[6 * j + i] = v; }
static void swap_d(double* a, double* b) { const double t = *a; *a = *b; *b = t; }

/* d2J_dX2 and d2J_dZdX cov_z d2J_dZdX^T from the 16 sums of cov6_kernel (+ the pair counts), then
 * cov6 = 0.01 inv(H) M inv(H) (Gauss-Jordan with partial pivoting, fp64, fixed order) */
int dpg_cov6_from_sums(const double* sm, int64_t nh, int64_t nb, double cov6[36]) {
    double H[36] = {0}, M[36] = {0};
    enum { X = 0, Y = 1, Z = 2, A = 3, B = 4, C = 5 };
    sym6(H, X, X, 2.0 * (double)nh); sym6(H, Y, Y, 2.0 * (double)nh); sym6(H, Z, Z, 2.0 * (double)nh);
    sym6(H, X, A, sm[0]); sym6(H, Y, A, sm[1]); sym6(H, A, A, sm[2]); sym6(H, Z, B, sm[3]); sym6(H, Z, C, sm[4]);
    sym6(H, B, B, sm[5]); sym6(H, B, C, sm[6]); sym6(H, C, C, sm[7]);
    sym6(M, X, X, 8.0 * (double)nb); sym6(M, Y, Y, 8.0 * (double)nb); sym6(M, Z, Z, 8.0 * (double)nb);
    sym6(M, X, A, sm[8]); sym6(M, Y, A, sm[9]); sym6(M, A, A, sm[10]); sym6(M, Z, B, sm[11]); sym6(M, Z, C, sm[12]);
    sym6(M, B, B, sm[13]); sym6(M, B, C, sm[14]); sym6(M, C, C, sm[15]);
    double I[36] = {0};
    for (int i = 0; i < 6; ++i) I[7 * i] = 1.0;
    for (int c = 0; c < 6; ++c) {
        int p = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(H[6 * r + c]) > fabs(H[6 * p + c])) p = r;
        if (!(fabs(H[6 * p + c]) > 0.0)) return DPG_ERR_NUMERIC;
        if (p != c)
            for (int k = 0; k < 6; ++k) { swap_d(&H[6 * p + k], &H[6 * c + k]); swap_d(&I[6 * p + k], &I[6 * c + k]); }
        const double d = H[6 * c + c];
        for (int k = 0; k < 6; ++k) { H[6 * c + k] /= d; I[6 * c + k] /= d; }
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = H[6 * r + c];
            if (f == 0.0) continue;
            for (int k = 0; k < 6; ++k) { H[6 * r + k] -= f * H[6 * c + k]; I[6 * r + k] -= f * I[6 * c + k]; }
        }
    }
    double T1[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += I[6 * i + k] * M[6 * k + j];
            T1[6 * i + j] = acc;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc += T1[6 * i + k] * I[6 * k + j];
            cov6[6 * i + j] = 0.01 * acc;
        }
    return DPG_OK;
}
