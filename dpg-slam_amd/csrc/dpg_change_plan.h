// dpg_change_plan.h -- the host plan of one dpg_execute_dpg_chain (dpg_change_plan.cpp; plain C++, no
// device call, private): chain, candidates, the window and its reuse, each chain node's bit-plane.
// node_frame is here because the plan and the store's frame cache must agree on it.
#ifndef DPG_CHANGE_PLAN_H
#define DPG_CHANGE_PLAN_H

#include <stdint.h>

#include <vector>

#include "../../include/dpg_slam_c.h"

#pragma GCC visibility push(hidden)   // nothing here is exported from the library

constexpr int kChainMax = 15;   // chain nodes, and bit-plane pairs of a window word (bits 30, 31: the submap)

struct Box { int32_t x0, y0, w, h; };   // a window of cells: first keys, extent

// The window kept across calls: chain grids of nodes still in the chain (same pose) stay as planes,
// only the new chain node is rasterised.  slot_node[q]: the node whose grid plane q holds, -1 free.
struct ChangeKept {
    Box win{};
    bool win_valid = false;
    int32_t slot_node[kChainMax] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    float slot_pose[kChainMax][3] = {};
};

struct ChangePlan {
    int32_t n_chain = 0, n_rast = 0;
    int32_t chain[kChainMax];        // chain node ids, ascending
    int32_t slot[kChainMax];         // [chain]: the node's plane
    int32_t rast[kChainMax];         // [n_rast]: chain indices whose grid is (re)rasterised
    float cframe[kChainMax][8];      // [chain]: frames at the CHAIN poses (node_frame)
    std::vector<int32_t> cand;       // candidate node ids, node order
    int32_t chain_sep = 0;           // 1: some chain pose differs from that node's estimate
    Box need{}, win{};               // what the chain's rays need; the window of this call
    bool reuse = false;              // the kept window holds `need`: planes in keep_mask stay
    uint32_t keep_mask = 0, chain_bits = 0;
    ChangeKept kept;                 // the kept state after this call (the caller commits it)
};

// math_utils::AngleMod<float> (math_utils.h:13-16)
float angle_mod_f(float a);
// node frame of the pose e and the laser's mount: the lidar pose in the map (transformPoint(laser, node pose),
// dpg_node.cc:34-36) and Rotation2Df(+-a) from the host libm: f = (lmx, lmy, cos a, sin a, cos -a, sin -a, 0, 0)
void node_frame(const float laser[3], const float* e, float* f);

// The plan of a call over nodes [0, V) whose last cur_len are the current pass.  chain_poses (NULL: the
// estimates): the chain nodes' grid poses; active [V]: the host mirror of the node activity; rmax_beam [V]: each
// node's largest range.  DPG_OK, DPG_ERR_ARG (a non-finite chain pose) or DPG_ERR_SIZE (a window above 2^28 cells).
int dpg_change_plan(const dpg_change_params& p, int64_t V, int64_t cur_len, const float* est, const float* chain_poses,
                    const uint8_t* active, const float* rmax_beam, const ChangeKept& kept, ChangePlan& pl);

#pragma GCC visibility pop

#endif
