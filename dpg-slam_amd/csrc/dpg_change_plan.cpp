// dpg_change_plan.cpp -- the planning half of dpg_execute_dpg_chain as one pure function, and the node
// frame it shares with the store's frame cache (plain C++, no device call).  Built with
// -ffp-contract=off: fp32 expressions stand as the reference writes them, the trig is the oracle's libm.
#include "dpg_change_plan.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

float angle_mod_f(float a) {
    double ad = (double)a;
    ad -= (M_PI * 2.0) * rint(ad / (M_PI * 2.0));
    return (float)ad;
}

void node_frame(const float laser[3], const float* e, float* f) {
    const float th = e[2];
    const float c0 = cosf(th), s0 = sinf(th), ns0 = -s0;
    const float lx = e[0] + (c0 * laser[0] + ns0 * laser[1]);
    const float ly = e[1] + (s0 * laser[0] + c0 * laser[1]);
    const float a = angle_mod_f(th + laser[2]);
    f[0] = lx; f[1] = ly; f[2] = cosf(a); f[3] = sinf(a); f[4] = cosf(-a); f[5] = sinf(-a); f[6] = 0.f; f[7] = 0.f;
}

int dpg_change_plan(const dpg_change_params& p, int64_t V, int64_t cur_len, const float* est, const float* chain_poses,
                    const uint8_t* active, const float* rmax_beam, const ChangeKept& kept, ChangePlan& pl) {
    pl = ChangePlan();
    pl.kept = kept;
    const int64_t n_past = V - cur_len;
    const int64_t chain_n = std::min<int64_t>(cur_len, p.current_pose_chain_len);
    pl.n_chain = (int32_t)chain_n;
    for (int64_t k = 0; k < chain_n; ++k) pl.chain[k] = (int32_t)(V - chain_n + k);
    // the pose of chain node k for its grid and the proximity search: the caller's chain pose
    // (current_pass_nodes_, dpg_slam.cc:591-620,646-668) or the node's estimate
    auto cpose = [&](int64_t k) { return chain_poses ? chain_poses + 3 * k : est + 3 * (int64_t)pl.chain[k]; };
    // candidates: active past nodes within the proximity threshold of a chain node (:646-668)
    for (int64_t j = 0; j < n_past && chain_n > 0; ++j) {
        if (!active[j]) continue;
        for (int64_t k = 0; k < chain_n; ++k) {
            const float* c = cpose(k);
            const float dx = c[0] - est[3 * j], dy = c[1] - est[3 * j + 1];
            if (sqrtf(dx * dx + dy * dy) <= p.distance_threshold_for_local_submap_nodes) { pl.cand.push_back((int32_t)j); break; }
        }
    }
    if (chain_n == 0) return DPG_OK;   // no pose chain: no window, the kept state stays
    for (int64_t k = 0; k < chain_n; ++k) {
        const float* c = cpose(k);
        const int32_t v = pl.chain[k];
        if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) ||
            !std::isfinite(est[3 * v]) || !std::isfinite(est[3 * v + 1]) || !std::isfinite(est[3 * v + 2]))
            return DPG_ERR_ARG;
        node_frame(p.laser, c, pl.cframe[k]);
        if (memcmp(c, est + 3 * v, 3 * sizeof(float)) != 0) pl.chain_sep = 1;
    }
    // window: every chain ray stays within its longest range of the lidar
    double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
    for (int64_t k = 0; k < chain_n; ++k) {
        const double r = rmax_beam[pl.chain[k]];
        xlo = std::min(xlo, pl.cframe[k][0] - r); xhi = std::max(xhi, pl.cframe[k][0] + r);
        ylo = std::min(ylo, pl.cframe[k][1] - r); yhi = std::max(yhi, pl.cframe[k][1] + r);
    }
    Box& need = pl.need;
    need.x0 = (int32_t)floor(xlo / p.occ_grid_resolution) - 4;
    need.y0 = (int32_t)floor(ylo / p.occ_grid_resolution) - 4;
    need.w = (int32_t)ceil(xhi / p.occ_grid_resolution) + 4 - need.x0 + 1;
    need.h = (int32_t)ceil(yhi / p.occ_grid_resolution) + 4 - need.y0 + 1;
    ChangeKept& K = pl.kept;
    const Box& w0 = K.win;
    pl.reuse = K.win_valid && need.x0 >= w0.x0 && need.y0 >= w0.y0 && need.x0 + need.w <= w0.x0 + w0.w &&
               need.y0 + need.h <= w0.y0 + w0.h;
    if (!pl.reuse) {   // new window with a margin, so the next chain nodes usually still fit
        const int32_t m = (int32_t)ceil(4.0 / p.occ_grid_resolution);
        Box nw{need.x0 - m, need.y0 - m, need.w + 2 * m, need.h + 2 * m};
        if ((int64_t)nw.w * nw.h > (int64_t)1 << 28) nw = need;
        if ((int64_t)nw.w * nw.h > (int64_t)1 << 28) return DPG_ERR_SIZE;
        K.win = nw; K.win_valid = true;
        for (int q = 0; q < kChainMax; ++q) K.slot_node[q] = -1;
    }
    pl.win = K.win;
    // bit-plane slots: a chain node keeps its plane while it stays in the chain with the same pose
    for (int64_t k = 0; k < chain_n; ++k) pl.slot[k] = -1;
    for (int q = 0; q < kChainMax; ++q) {
        const int32_t v = K.slot_node[q];
        if (v < 0) continue;
        const int64_t k = v - (V - chain_n);
        if (k >= 0 && k < chain_n && memcmp(K.slot_pose[q], cpose(k), 3 * sizeof(float)) == 0) {
            pl.slot[k] = q; pl.keep_mask |= 3u << (2 * q);
        } else {
            K.slot_node[q] = -1;
        }
    }
    for (int64_t k = 0; k < chain_n; ++k) {
        if (pl.slot[k] < 0) {
            int q = 0;
            while (K.slot_node[q] >= 0) ++q;   // chain_n <= kChainMax planes: always one free
            K.slot_node[q] = pl.chain[k];
            memcpy(K.slot_pose[q], cpose(k), 3 * sizeof(float));
            pl.slot[k] = q;
            pl.rast[pl.n_rast++] = (int32_t)k;
        }
        pl.chain_bits |= 3u << (2 * pl.slot[k]);
    }
    return DPG_OK;
}
