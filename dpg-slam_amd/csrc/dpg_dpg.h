// dpg_dpg.h -- the DPG node store (struct dpg_dpg) as dpg_store.hip, dpg_change.hip, dpg_grid.hip and
// dpg_loc.hip see it, and the frozen map (struct dpg_fmap) of dpg_loc.hip, dpg_track.hip and dpg_refine.hip (private,
// C++).  Every array releases itself; kernels take the view DS (make_ds).
#ifndef DPG_DPG_H
#define DPG_DPG_H

#include "dpg_change_plan.h"
#include "dpg_ctx.h"

#pragma GCC visibility push(hidden)

struct Ctl {                     // device counters, fetched once at the end of a call
    unsigned long long chain_cells, samples, oob, n_added, n_removed, sect_off, nodes_off, pad;
    int32_t n_acc, uncovered_lo, uncovered_hi, pad2;
};
struct OccCtl { unsigned long long samples, oob, hits, direct, flushed, beams, pad0, pad1; };

// the staging block of a call, int32 words, one H2D copy: chain 16 | slot 16 | rast 16 | chain frames 128 | candidates
constexpr int64_t kStageChain = 0, kStageSlot = 16, kStageRast = 32, kStageFrames = 48, kStageCand = 48 + 128;

struct DS {                      // device view of the node store + per-call scratch
    const int64_t* off;
    const float2* plaser;
    const float* range;
    uint8_t* label;
    const uint8_t* sector;
    const float4* geom;          // amin, amax, rmax, angle_inc
    uint32_t* sect;              // per node: bit s = sector s active
    uint32_t* active;
    const float4* frame;         // [2V]: (lmx, lmy, cos a, sin a), (cos -a, sin -a, 0, 0)
    uint32_t* grid;
    int32_t* first;
    const int32_t* chain;        // chain node ids
    const int32_t* slot;         // [chain]: bit-plane slot of chain node k (bits 2 slot, 2 slot + 1)
    const int32_t* rast;         // chain indices whose grid is (re)rasterised this call
    const float4* cframe;        // [2 chain]: frames of the chain nodes at their CHAIN poses (grids)
    int32_t chain_sep;           // 1: some chain pose differs from that node's estimate
    uint32_t chain_bits;         // planes of the current chain nodes
    uint32_t keep_mask;          // planes kept from the previous call (window reused)
    int32_t rebuild;             // 1: window (re)built, every plane starts empty
    const int32_t* cand;         // candidate node ids, node order
    int32_t* cand_cnt;
    int32_t* acc;
    uint32_t* bins;              // [chain][bin_words]
    int32_t* inrange;            // [chain]
    int32_t* commit;             // [chain + 1]: flags, [chain] = mask
    uint8_t* added;              // [chain][max_beams]
    uint16_t* rmask;             // [n_cand][max_beams]
    float2* removed_xy;
    Ctl* ctl;
    double res, inv_res;
    int32_t max_beams, n_chain, n_cand, bin_words, total_bins, num_sectors;
    float min_pct;
    double change_thr, cover_thr;
    Box box;
};

// dpg_loc.hip's field, its pooled form and the search buffers: a member of the store, empty until first asked for
struct LocRec { int32_t score, a, dx, dy; };   // a scored candidate; score < 0: none
struct DpgLoc {
    DevBuf<uint8_t> field, pool_tmp, pooled;   // F [h][w], the row-pooled F, P [h + s - 1][w + s - 1]
    DevBuf<float> rot, cloud;                  // [A][2], [n_pts][2]
    DevBuf<int2> keys;                         // [A][n_pts] field indices of the points at shift (-hx, -hy)
    DevBuf<int32_t> vol;                       // [A][nby][nbx] bounds; the score volume of the diagnostic
    DevBuf<int2> tile_best, seeds, entries;    // per (angle, tile) and per angle (bound, block); (a, block) lists
    DevBuf<LocRec> partial, rec;               // per workgroup bests of a fine launch; [0] seeds', [1] overall, [2] at the guess
    DevBuf<uint32_t> counter;                  // the frontier's size
    DevEvent ev[4];
};

struct dpg_dpg {
    dpg_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    int device = 0;
    dpg_change_params p{};
    int64_t V = 0, B = 0;
    int32_t max_beams = 0;
    std::vector<int64_t> off;
    std::vector<float> geom;          // [V][4]
    std::vector<float> rmax_beam;     // largest range of each node's beams (window size)
    std::vector<uint8_t> active_h;    // host mirror of the node activity
    std::vector<float> h_pose;        // [V][3] pose bits the cached frames were computed from (NaN: none)
    PinBuf<float> h_frames;           // [V][8] cached node frames, pinned (see upload_frames)
    PinBuf<unsigned char> h_app;      // pinned staging of dpg_dpg_append's uploads
    // pinned: the staging block of a call (kStage*), the node activity and commit flags read back
    PinBuf<int32_t> h_stage;
    PinBuf<uint32_t> h_act;
    PinBuf<int32_t> h_commit;
    ChangeKept kept;                  // the window and planes kept across calls (dpg_change_plan.h)
    DevBuf<int64_t> d_off;
    DevBuf<float2> d_plaser;
    DevBuf<float> d_range;
    DevBuf<uint8_t> d_label, d_sector;
    DevBuf<float4> d_geom, d_frame;
    DevBuf<uint32_t> d_sect, d_active, d_grid, d_bins;
    DevBuf<int32_t> d_first, d_stage, d_cand_cnt, d_acc, d_inrange, d_commit;
    DevBuf<uint8_t> d_added;
    DevBuf<uint16_t> d_rmask;
    DevBuf<float2> d_removed, d_map_out;
    DevBuf<Ctl> d_ctl;
    DevBuf<int64_t> d_counts, d_base;
    // dpg_occupancy_grid / dpg_dpg_beam_geometry: buffers of their own, empty until the first request
    DevBuf<int32_t> d_occ_cnt, d_occ_nodes;   // [hits | misses], the active node list
    DevBuf<int8_t> d_occ_out;
    DevBuf<OccCtl> d_occ_ctl;
    DevBuf<float2> d_geo;                     // [lidar positions | end points]
    DpgLoc loc;                               // dpg_map_localize's field and search buffers (dpg_loc.hip)
    PinBuf<Ctl> h_ctl;
    DevEvent ev[2];
};

// A frozen map (dpg_fmap_*): a likelihood field with its box and resolution in buffers of its own, a
// child of the context that keeps no reference to the store it was taken from.  dpg_loc.hip creates,
// saves, loads and searches it; dpg_track.hip tracks batches of scans against it, dpg_refine.hip
// refines their poses on it.
struct TrackRec { LocRec win; int32_t score_at_guess, pad[3]; };   // a scan's record as the device leaves it
struct dpg_fmap {
    dpg_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    int device = 0;
    int32_t box[4] = {0, 0, 0, 0};            // x0, y0, w, h
    double res = 0.0;
    float sigma = 0.f;                        // how F was made: metadata, not read by any search
    int32_t kernel_radius = 0, occupied_min = 0;
    DevBuf<uint8_t> field;                    // F [h][w]
    DevBuf<uint8_t> pooled[6];                // P at shift 1 .. 5, pooled from F at first use and kept
    bool have_pooled[6] = {false, false, false, false, false, false};
    DpgLoc loc;                               // dpg_fmap_localize's search buffers (its field and pooled stay empty)
    // dpg_fmap_track: the call's one upload (pinned, then device), the (scan, angle) bests, the scores at
    // the guesses and the records
    PinBuf<unsigned char> h_in;
    DevBuf<unsigned char> d_in;
    DevBuf<LocRec> part;
    DevBuf<int32_t> at_guess;
    DevBuf<TrackRec> recs;
    PinBuf<TrackRec> h_recs;
    DevEvent track_ev[2];                     // around the two launches of the last call
    float track_ms = 0.f;
    // dpg_fmap_refine / dpg_fmap_track_refine (dpg_refine.hip): the call's one block of results on the
    // device and pinned -- [the track records |] the refine records [| the trace]; the upload goes
    // through h_in and d_in
    DevBuf<unsigned char> r_out;
    PinBuf<unsigned char> h_rout;
    DevEvent refine_ev[2];                    // around the refinement launch of the last call
    float refine_ms = 0.f;
    int64_t cells() const { return (int64_t)box[2] * box[3]; }
};

// ---- dpg_track.hip: dpg_fmap_track in the stages that dpg_fmap_track_refine (dpg_refine.hip) shares ----
// one scan of the batch as the kernels read it: its points [begin, end) of the batch's cloud array and
// the keys (cx, cy) of its guess
struct TrackScan { int64_t begin, end; int32_t cx, cy, pad[2]; };
// a checked request staged in m->h_in, one block: scans [B] | rot [B][A][2] | the points from offsets[0] on
struct TrackStage {
    dpg_track_params P;
    int64_t B = 0, A = 0, total = 0;
    size_t o_scan = 0, o_rot = 0, o_pts = 0, n_in = 0;
    TrackScan* scans = nullptr;               // in m->h_in
    float* rot = nullptr;
};
// every check of dpg_fmap_track's contract, nothing touched; B = 0 passes
int track_check(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                const dpg_track_params* p, const void* out, const char* who);
// B > 0, checked: makes the map's device current, waits for its stream and fills h_in
int track_stage(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                const dpg_track_params* p, const char* who, TrackStage& st);
// a map with cells: the two launches over the block uploaded at d_in, the records to d_recs [B]
int track_launch(dpg_fmap* m, const TrackStage& st, TrackRec* d_recs, const char* who);
// out[B] from the device's records (recs NULL: an empty map's)
void track_results(const dpg_fmap* m, const TrackStage& st, const float* guesses, const TrackRec* recs, dpg_track_result* out);

// ---- dpg_store.hip ----
DS make_ds(dpg_dpg* d);
// Node frames (node_frame) cached per node, keyed by the pose bits: only nodes whose estimate changed
// are recomputed and uploaded.  active_only: inactive nodes are skipped (executeDPG and the grid never
// read their frames); their stale pose bits stay in h_pose until the map lists need them
int upload_frames(dpg_dpg* d, int64_t V, const float* est, bool active_only = false);

// ---- dpg_grid.hip: the occupancy grid of the active nodes, for dpg_occupancy_grid and the localiser ----
struct GridPlan {
    double res = 0.0;
    int32_t variant = 0, box[4] = {0, 0, 0, 0};   // occ_raster_kernel's launch variant; x0, y0, w, h
    int64_t cells = 0;
    std::vector<int32_t> nodes;                   // the active nodes
};
// checks the request, brings the frames up to date and takes the box over the active nodes
int grid_plan(dpg_dpg* d, int64_t V, const float* est, const dpg_grid_params& gp, GridPlan& g);
// the device run of a plan with cells > 0, waited for: hits at d_occ_cnt.p, misses grid_pitch(cells) further,
// the occupancy bytes (want_occ) at d_occ_out.p; fills info's counters and ms_kernels
int grid_run(dpg_dpg* d, const GridPlan& g, bool want_occ, dpg_grid_info* info);
inline int64_t grid_pitch(int64_t cells) { return (cells + 63) & ~(int64_t)63; }   // misses start on a 256-B boundary

#pragma GCC visibility pop

#endif
