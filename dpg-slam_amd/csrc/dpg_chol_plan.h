// dpg_chol_plan.h -- what the Cholesky solver's host planner (dpg_chol_plan.cpp, plain C++) and its
// kernels and driver (dpg_chol*.hip, dpg_chol_dev.h) must agree on (private): the records the plan writes and the
// kernels follow, the tile / panel constants, the per-front cost model (also the symbolic
// analysis's order choice, dpg_chol_sym.cpp), and CholPlan, everything one plan produces.
#ifndef DPG_CHOL_PLAN_H
#define DPG_CHOL_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "dpg_chol.h"

#ifdef __HIPCC__
#define DPG_HD __host__ __device__
#else
#define DPG_HD
#endif

namespace dpg_chol {

constexpr int kT = 256;     // threads per front workgroup
constexpr int kNB = 48;     // factorization panel width (scalar columns, 16 3x3 blocks)
constexpr int kSB = 64;     // triangular-solve diagonal block
constexpr int kCT = 32;     // assembly column tile
constexpr int kUT = 32;     // trailing-update tile (rows and columns)
constexpr int kDL = kSB + 1;   // leading dimension of D in the inverse path (transposed stores conflict-free)
constexpr int kMaxSeg = 32;   // row segments held in LDS (a front with more waits for its parent, then takes every row)
// L11^-1 (chol_inv_l11)
constexpr int kInvCols = 4;              // columns (waves) per workgroup
constexpr int kInvMaxQ = 3;              // rows per lane
// fused DAG factorization (chol_factor_dag)
constexpr int kFT = 512;    // threads per front workgroup
constexpr int kFNB = 24;    // panel width (scalar columns = 8 3x3 blocks)
constexpr int kSmall = 96;  // fronts up to this many rows are assembled + factored entirely in LDS
constexpr int kMaxCh = 8;   // ... if they have at most this many children
constexpr int kGmax = 32;    // largest team (workgroups per front)

// task records of the task-list kernels (the layout of HIP's int2 / int4)
struct alignas(8) Task2 { int32_t x, y; };
struct alignas(16) Task4 { int32_t x, y, z, w; };

struct SnDev {
    int32_t c0, k, r, nchild;   // k, r in 3x3 blocks
    int64_t front_off;          // doubles
    int64_t rows_off;           // into rows / relmap
    int64_t child_off;          // into child_list
    int64_t omap_off;
    int64_t acc_off;            // doubles (3r pending row updates of the forward solve)
    int32_t omap_n, parent;     // parent supernode, -1 at a root
    int32_t G, need;            // fused factorization: team size, sum of the children's team sizes
    int32_t ftask;              // large fronts: first tile task
    int32_t inv;                // L11^-1 of the front at linv + inv (k3 x k3, column-major), -1: none
    int32_t seg_off, seg_n;     // backward solve: the row segments by owning supernode (SolveSeg)
};

// A front's rows (ascending positions) fall into segments owned by its ancestors, the parent's
// first: the backward solve takes each segment's x as soon as its owner has published it.
struct SolveSeg { int32_t sn, t0, t1, pad; };   // rows [t0, t1) (blocks) owned by supernode sn

struct OEnt {                   // one upper 3x3 block of H -> its front position
    int32_t u;                  // block index in the packed hb buffer
    int16_t a, b;               // local block row / column in the front
    int32_t tr, pad;            // 1: the front wants H(lo,hi)^T
};

// level path, assembly: one task per (front, kCT-column tile)
struct AsmTask {
    int32_t s, c0;              // front, first column of the tile
    int32_t om_b, om_e;         // omap entries whose block column meets the tile
    int32_t ch_off, ch_cnt;     // into AsmChild: the children with columns in the tile
};
struct AsmChild { int32_t c, ja, jb, pad; };

// fused path, per (large front, tile): the H blocks and the children's column ranges that land in the tile
struct FTask { int32_t om_b, om_e, ch_off, ch_cnt; };
struct FChild { int32_t ja, jb, k, r; int64_t front_off, rows_off; };
// a small front's per-child record in LDS (its size is part of the LDS budget)
struct ChMeta { int64_t front_off, acc_off, rows_off; int32_t k, r; };

static_assert(sizeof(Task2) == 8 && alignof(Task2) == 8 && sizeof(Task4) == 16 && alignof(Task4) == 16, "int2 / int4 layout");
static_assert(sizeof(SnDev) == 88 && alignof(SnDev) == 8 && sizeof(OEnt) == 16 && alignof(OEnt) == 4, "record layout");
static_assert(sizeof(SolveSeg) == 16 && sizeof(AsmTask) == 24 && sizeof(AsmChild) == 16 && alignof(AsmTask) == 4, "record layout");
static_assert(sizeof(FTask) == 16 && sizeof(FChild) == 32 && alignof(FChild) == 8 && sizeof(ChMeta) == 32, "record layout");

// LDS carve of the factorization phase (doubles): panel [kFNB][Rp] with row offset `off` so that
// trailing rows start 32-B aligned, L_top column-major [kFNB][kFNB], 1/diag, step scratch.
DPG_HD inline int fused_rp(int R, int off) { return (R + off + 3) & ~3; }
constexpr int kFScr = kFNB * kFNB + 8 * (kFNB / 3) + 384;   // L_top, 3x3 inverses, POTRF exchange
DPG_HD inline size_t fused_lds_doubles(int m3, int k3, bool db) {
    // right-hand side | scratch | one or two panel buffers (the first also holds the assembly tile)
    const size_t large = ((m3 + 1) & ~1) + kFScr + (db ? 2 : 1) * (size_t)kFNB * fused_rp(m3, 3);
    (void)k3;
    const size_t small = m3 <= kSmall ? (size_t)m3 * m3 + m3 + (kMaxCh * sizeof(ChMeta) + kMaxCh * (kSmall / 3) * 4 + 7) / 8 : 0;
    return 2 + std::max(small, large);
}

// ---- the per-front cost model of the fused factorization ----
// A front of m3 rows, k3 pivot columns and nchild children is factored in LDS by one workgroup
// (small_front) or by a team (large_front): the planner sizes the team and orders the tickets by
// it, and the symbolic analysis picks the elimination order by the same estimate.
inline bool front_is_small(int32_t m3, int32_t nchild) { return m3 <= kSmall && nchild <= kMaxCh; }
// workgroups of the front's team: one per pivot and update tile, at most kGmax
inline int32_t front_team_size(int32_t m3, int32_t k3, int32_t nchild) {
    return front_is_small(m3, nchild) ? 1 : std::min(kGmax, (k3 + kFNB - 1) / kFNB + (m3 - k3 + kFNB - 1) / kFNB);
}
// estimated time (us, fitted to tools/chol_bench_t's per-front log: a small front's time grows
// with its columns -- ~0.9 us each for the in-LDS factorization -- as well as its rows; a large
// front's with its chain of kFNB-column panels)
inline double front_est_us(int32_t m3, int32_t k3, int32_t nchild) {
    return front_is_small(m3, nchild) ? 4.0 + 0.06 * m3 + 0.9 * k3 : 10.0 + 20.0 * ((k3 + kFNB - 1) / kFNB);
}

// Everything one plan produces, for the analysis S of a graph of n nodes and its pairs: the arrays
// the upload copies to the device, the launch parameters the driver reads, and the scratch of the
// build (kept between builds: the incremental graph rebuilds per update).  Host memory only.
struct CholPlan {
    struct Blk { int32_t row, u, tr; };   // an upper block of H in its column's bucket
    struct Blk4 { int32_t row, col, u, tr; };
    struct Step { int32_t panel_off, panel_cnt, rpt /* panel rows / kT, rounded up */, max_rows, upd_off, upd_cnt; };
    struct Level { int32_t asm_off, asm_cnt; size_t lds_asm; std::vector<Step> steps; };

    // scratch
    std::vector<int64_t> colptr;
    std::vector<Blk> ent;
    std::vector<Blk4> byrow;
    std::vector<int32_t> lidx, lstamp;
    std::vector<int64_t> om_ptr, om_cur;
    std::vector<double> prio, hgt;
    std::vector<int32_t> hcnt;
    std::vector<std::pair<double, int32_t>> key;
    std::vector<int32_t> cuts;
    std::vector<int32_t> tcnt, tfill;   // per-tile child counts / fill cursors of one large front
    std::vector<char> tused;
    // colptr / ent built ahead by dpg_chol_plan_prebucket (the incremental prepare runs it beside
    // the symbolic derivation) for a graph of blocks_n nodes and blocks_np pairs; the next plan takes them
    bool blocks_ready = false;
    int64_t blocks_n = -1, blocks_np = -1;

    // the device arrays
    std::vector<OEnt> omap;
    std::vector<SnDev> sns;
    std::vector<FTask> ftasks;          // large fronts: per-tile assembly lists
    std::vector<FChild> fchild;
    std::vector<SolveSeg> segs;
    std::vector<int32_t> fo;            // forward solve: fronts in the tickets' order
    std::vector<int32_t> order_fac;     // fused factorization tickets (front * 64 + member)
    std::vector<int32_t> bwd;           // backward solve: fronts by descending height
    std::vector<AsmTask> asm_t;         // level path
    std::vector<AsmChild> asm_c;
    std::vector<Task2> panel_t;
    std::vector<Task4> upd_t;
    std::vector<Task2> dblocks;         // (front, jb) of every diagonal block
    std::vector<Task2> inv_t;           // chol_inv_l11 tasks (front, first column)

    // sizes and launch parameters
    int64_t n = 0, nnzb_upper = 0;
    int64_t acc_total = 0;              // doubles of pending row updates
    int64_t n_tickets = 0;
    int64_t n_inv_tasks = 0, linv_total = 0;
    size_t lds_inv = 0;
    int64_t n_dblocks = 0;
    bool use_dinv = false;              // opts.solve_dinv: inverted diagonal blocks (measured slower)
    size_t sync_bytes = 0;              // the sync words (layout: dpg_chol_dev.h)
    size_t lds_solve_max = 0;
    int32_t solve_stage = 0;   // R: LDS staging region of the solves, doubles (Stage)
    int32_t solve_maxseg = 0;  // backward: fronts with more row segments wait for the parent (<= kMaxSeg)
    // fused DAG factorization + forward solve (used when every front fits its LDS budget)
    bool fused = false;
    size_t lds_fused = 0;
    bool fused_db = true;               // two LDS panel buffers for the chain
    // level path: the per-level launch plan
    std::vector<Level> levels;
    std::vector<int32_t> level_ptr;
    int64_t n_launches = 0;
    std::vector<int32_t> cur_G;         // team sizes (written by tracked plans only: partial refactorization)
};

// H's upper blocks bucketed by column position, ahead of the plan of a graph with n nodes and these
// pairs whose analysis will carry the ordering pos / perm (the plan's first stage)
void dpg_chol_plan_prebucket(CholPlan& P, int64_t n, const int32_t* pos, const int32_t* perm, const int32_t* pair_lo,
                             const int32_t* pair_hi, int64_t n_pairs);
// The plan of analysis S under the options o; track: keep the team sizes for partial
// refactorization.  No device call; DPG_OK or a DPG_ERR_* code.
int dpg_chol_plan_build(CholPlan& P, const dpg_chol_sym& S, const dpg_chol_opts& o, bool track, int64_t n,
                        const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs);

// ---- partial refactorization: which fronts keep the last factorization's values (dpg_chol_solve_partial) ----
struct PartialPick {
    std::vector<uint8_t> keep;    // [ns] 1: the front keeps its values
    std::vector<int32_t> old;     // [ns] a kept front's front in the old analysis, else -1
    // the kept fronts (buf 0) and their pending forward-solve updates (buf 1) the new layout moved
    std::vector<int64_t> runs;    // {src, dst, doubles, buf} per run, adjacent runs merged
    int64_t kept = 0, moved = 0, max_run = 0;   // fronts kept, doubles moved, the longest run
};
// The pick for the new analysis S over the old one O (O's order a prefix of S's: the caller checks)
// with their team sizes cur_G / fac_G and the nodes whose H blocks changed.  A front is kept when it has
//   * the same columns (same first column, same count: positions are stable between reorders), the
//     same rows, the same children (by first column, in order: the extend-add order) and the same
//     team size (the arithmetic order of the factorization kernel) as a front of O;
//   * no dirty node's column in it (its H blocks are then the same sums of the same factors at the
//     same linearization point: the caller's contract);
//   * no front below it that is not kept (its children's update matrices are unchanged).
// False -- refactor everything -- on a dirty node out of range, nothing kept, or more than 65535 runs.
bool dpg_chol_plan_partial(PartialPick& K, const dpg_chol_sym& S, const dpg_chol_sym& O, const std::vector<int32_t>& cur_G,
                           const std::vector<int32_t>& fac_G, const int32_t* dirty_nodes, int64_t n_dirty);

// ---- joint marginals: blocks of Sigma anywhere, from root paths of the factor (dpg_chol_joint) ----
// W_q = L^-1 E_q (E_q: the three unit columns of node q) is nonzero only on the pivot rows of the
// fronts from q's own to the root of its tree.  A query's slice of the compact W buffer holds
// those rows, front after front in path order, row-major [scalars][3]; two root paths share a
// suffix of equal length in both slices (from the lowest common front to the root; nothing when
// the nodes lie in different trees), and Sigma(i, j) is the 3x3 product of the two suffixes.
constexpr int kPB = 24;          // pivot block of the path solve (scalar columns)
constexpr int kPathLds = 2048;   // doubles: the path solve keeps its two vectors in LDS up to here (16 KiB)
constexpr int kPathGrid = 1024;  // workgroups of the path solve at most (each takes every kPathGrid-th query)
// rows per right-hand side of the path solve's vectors, and whether the two [3][ldv] vectors fit LDS
inline int path_ldv(int32_t max_front) { return (3 * max_front + 1) & ~1; }
inline bool path_in_lds(int32_t max_front) { return 6 * path_ldv(max_front) <= kPathLds; }

struct PathQuery { int32_t sn, row; int64_t w_off; };   // first front, the node's first scalar row in it, slice (doubles)
// one 3x3 block: the suffixes' starts in W (doubles) and their length in scalars; the block goes to
// out[o + r ld + c] (o >= 0) and its transpose to out[ot + c ld + r] (ot >= 0)
struct PathPair { int64_t a, b, o, ot; int32_t len, pad; };
static_assert(sizeof(PathQuery) == 16 && sizeof(PathPair) == 40 && alignof(PathPair) == 8, "record layout");

struct JointPlan {
    std::vector<int32_t> nodes;        // the distinct queried nodes, in order of first appearance
    std::vector<PathQuery> queries;    // parallel to nodes
    std::vector<int64_t> path_ptr;     // [nodes + 1] into path_sn / path_len
    std::vector<int32_t> path_sn;      // the fronts of each path, the node's own first
    std::vector<int32_t> path_len;     // their pivot scalars
    std::vector<int64_t> len;          // scalars of each path (the slice holds 3 len doubles)
    std::vector<PathPair> pairs;
    int64_t w_total = 0;               // doubles of the W buffer
    int64_t out_total = 0;             // doubles of the output
    int32_t ld = 3;                    // leading dimension of the output's blocks
    std::vector<int32_t> slot;         // scratch: node -> index in nodes, -1
};
// Sigma(pairs[q][0], pairs[q][1]) -> out[q][9] row-major.  Nodes must be in range (the caller checks).
void dpg_chol_plan_joint_pairs(JointPlan& J, const dpg_chol_sym& S, const int32_t* pairs, int64_t n);
// the joint covariance of nodes[0 .. n) -> out[3n][3n] row-major: every block on or above the block
// diagonal once, mirrored below
void dpg_chol_plan_joint_nodes(JointPlan& J, const dpg_chol_sym& S, const int32_t* nodes, int64_t n);

}  // namespace dpg_chol

#endif
