// dpg_loc.hip -- localisation of one scan in the active map (dpg_map_localize and its diagnostics):
// the likelihood field of the store's occupancy grid, its pooled form, and an exact branch-and-bound
// search over (angle, dx, dy).  The contract -- field, pooled field, keys, score, blocks, bound, tie
// order, search and statuses -- is the comment above dpg_loc_params in include/dpg_slam_c.h; the host
// halves (dpg_loc_params_default / _check, dpg_loc_rotations) are plain C in dpg_host.c, the
// smoothing bytes are dpg_csm_lut's.  The reference has no such stage.
// The same search runs on a frozen map (dpg_fmap_*, at the end of this file): a field kept in a
// handle of its own; both callers fill a View and call search().  The helpers the tracker
// (dpg_track.hip) shares -- the key rule, the winner's order and its tree -- are in dpg_loc_dev.h.
//
// Unlike the pair matcher (dpg_csm.hip) the table is the whole map, so it lives in global memory and
// is gathered through L2; LDS holds only a chunk of the scan's keys.  Kernels, in launch order:
//   loc_field_kernel    one thread per cell: the largest lut[d2] over the occupied cells of its R-disc
//   loc_pool_kernel     twice (rows, then columns): the s x s maximum as two s-wide maxima
//   loc_keys_kernel     one thread per (angle, point): the rotated point's field index at the
//                       window's first shift, or kKeyNone; every later kernel reads these
//   loc_bound_kernel    a workgroup = one angle and a 64 x 4 tile of blocks, a thread = one block,
//                       lanes along bx: the keys pass through LDS in chunks and are read as
//                       broadcasts, the bytes of P come through L2 (neighbouring lanes read s bytes
//                       apart on one row); also the tile's best block in the seed order
//   loc_seed_kernel     a workgroup per angle: the best of its tiles = the angle's seed
//   loc_fine_kernel     a thread = one candidate of a listed block (or of every block, for the score
//                       volume), against F; the workgroup's best candidate in the winner's order
//   loc_reduce_kernel   one workgroup: the best of the workgroups' candidates
//   loc_frontier_kernel one thread per block: bound >= best0 appends (angle, block) through one
//                       atomic counter; the list's order is free, the winner is an order-free maximum
//   loc_point_kernel    one workgroup: the score at the guess
// Orders are compared field by field (the keys do not fit 64 bits at the largest windows), in LDS
// trees, so no result depends on which thread or workgroup came first.  Every loop is bounded by the
// validated parameters, the box and n_pts; no workgroup waits for another.

#include <math.h>
#include <string.h>

#include <cmath>

#include <stdio.h>

#include "dpg_loc_dev.h"

namespace {

constexpr int kT = kLocT;             // threads per workgroup
constexpr int kChunk = kLocChunk;     // keys per LDS chunk (16 KiB)
constexpr int kTileX = 64, kTileY = 4;
static_assert(kTileX * kTileY == kT, "a thread per block of the tile");
constexpr int64_t kVolMax = (int64_t)1 << 29;
constexpr int64_t kItemMax = (int64_t)1 << 36;

struct Stencil {
    uint8_t lut[64];   // [d2], d2 <= R^2 <= 49
    int32_t R, occupied_min;
};

struct Dims {
    int32_t w, h, pw, ph;     // F [h][w], P [ph][pw]
    int32_t s, shift;
    int32_t hx, hy, ha;
    int32_t nbx, nby, nblk;   // blocks per angle
    int32_t n_pts;
    int32_t tiles_x, n_tiles;
};

__global__ __launch_bounds__(kT) void loc_field_kernel(const int8_t* occ, uint8_t* F, int32_t w, int32_t h, Stencil st) {
    const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (c >= (int64_t)w * h) return;
    const int x = (int)(c % w), y = (int)(c / w);
    const int R = st.R;
    int best = 0;
    for (int oy = -R; oy <= R; ++oy) {
        const int yy = y + oy;
        if ((unsigned)yy >= (unsigned)h) continue;
        for (int ox = -R; ox <= R; ++ox) {
            const int xx = x + ox, d2 = ox * ox + oy * oy;
            if ((unsigned)xx >= (unsigned)w || d2 > R * R) continue;
            // 0 <= yy < h, 0 <= xx < w: inside occ; d2 <= 49 < 64
            if ((int)occ[(int64_t)yy * w + xx] >= st.occupied_min) best = max(best, (int)st.lut[d2]);
        }
    }
    F[c] = (uint8_t)best;
}

// out[y][px] = max over i < s of in[y][px - (s - 1) + i] (ROWS), out [rows][wi + s - 1], or
// out[py][x] = max over j < s of in[py - (s - 1) + j][x] (!ROWS), out [hi + s - 1][wi]
template <bool ROWS>
__global__ __launch_bounds__(kT) void loc_pool_kernel(const uint8_t* in, uint8_t* out, int32_t wi, int32_t hi, int32_t s) {
    const int32_t wo = ROWS ? wi + s - 1 : wi, ho = ROWS ? hi : hi + s - 1;
    const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (c >= (int64_t)wo * ho) return;
    const int px = (int)(c % wo), py = (int)(c / wo);
    int best = 0;
    for (int i = 0; i < s; ++i) {
        const int x = ROWS ? px - (s - 1) + i : px, y = ROWS ? py : py - (s - 1) + i;
        if ((unsigned)x >= (unsigned)wi || (unsigned)y >= (unsigned)hi) continue;
        best = max(best, (int)in[(int64_t)y * wi + x]);   // 0 <= x < wi, 0 <= y < hi
    }
    out[c] = (uint8_t)best;
}

// keys[a][i] = (kx + ox, ky + oy) with (ox, oy) = (cx - hx - x0, cy - hy - y0): the point's field
// index at the shift (-hx, -hy); grid (ceil(n_pts / kT), A)
__global__ __launch_bounds__(kT) void loc_keys_kernel(const float2* cloud, const float* rot, int2* keys, int32_t n_pts,
                                                      double res, int64_t ox, int64_t oy) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n_pts) return;
    const int a = blockIdx.y;
    keys[(int64_t)a * n_pts + i] = loc_key(cloud[i], rot[2 * a], rot[2 * a + 1], res, ox, oy);   // a < A, i < n_pts
}

// the seed order: higher bound, then the block nearer the window's centre, then the smaller index
__device__ __forceinline__ int64_t block_d2(const Dims& g, int32_t b) {
    const int64_t mx = 2 * ((int64_t)(b % g.nbx) * g.s - g.hx) + g.s - 1;
    const int64_t my = 2 * ((int64_t)(b / g.nbx) * g.s - g.hy) + g.s - 1;
    return mx * mx + my * my;
}
__device__ __forceinline__ bool seed_better(const Dims& g, int2 x, int2 y) {   // .x bound (-1: none), .y block
    if (x.x != y.x) return x.x > y.x;
    if (x.x < 0) return false;
    const int64_t dx = block_d2(g, x.y), dy = block_d2(g, y.y);
    if (dx != dy) return dx < dy;
    return x.y < y.y;
}
__device__ __forceinline__ int2 seed_reduce(const Dims& g, int2 mine, int2* sh) {
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int st = kT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st && seed_better(g, sh[threadIdx.x + st], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + st];
        __syncthreads();
    }
    return sh[0];
}

// grid (n_tiles, A)
__global__ __launch_bounds__(kT) void loc_bound_kernel(Dims g, const int2* keys, const uint8_t* P, int32_t* vol, int2* tile_best) {
    __shared__ int2 s_keys[kChunk];
    __shared__ int2 s_red[kT];
    const int tid = threadIdx.x, a = blockIdx.y, tile = blockIdx.x;
    const int bx = (tile % g.tiles_x) * kTileX + tid % kTileX, by = (tile / g.tiles_x) * kTileY + tid / kTileX;
    const bool active = bx < g.nbx && by < g.nby;
    // P's index of the block's first shift is the key plus this: <= 2 * 32768 + 2 * 32 per axis
    const int offx = bx * g.s + g.s - 1, offy = by * g.s + g.s - 1;
    const int2* kp = keys + (int64_t)a * g.n_pts;
    int32_t sum = 0;
    for (int c0 = 0; c0 < g.n_pts; c0 += kChunk) {
        __syncthreads();   // the chunk's last readers are done
        const int n = min(kChunk, g.n_pts - c0);
        for (int i = tid; i < n; i += kT) s_keys[i] = kp[c0 + i];   // c0 + i < n_pts
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int i = 0; i < n; ++i) {
                const int2 k = s_keys[i];   // |k| <= 2^27 or kKeyNone: the sums below stay in int32
                const int x = k.x + offx, y = k.y + offy;
                if ((unsigned)x < (unsigned)g.pw && (unsigned)y < (unsigned)g.ph) sum += (int32_t)P[(int64_t)y * g.pw + x];
            }
        }
    }
    const int32_t b = by * g.nbx + bx;
    if (active) vol[(int64_t)a * g.nblk + b] = sum;   // b < nblk
    const int2 best = seed_reduce(g, active ? make_int2(sum, b) : make_int2(-1, 0), s_red);
    if (tid == 0) tile_best[(int64_t)a * g.n_tiles + tile] = best;
}

// grid A: seeds[a] = (bound, block), entries[a] = (a, block)
__global__ __launch_bounds__(kT) void loc_seed_kernel(Dims g, const int2* tile_best, int2* seeds, int2* entries) {
    __shared__ int2 s_red[kT];
    const int a = blockIdx.x;
    int2 mine = make_int2(-1, 0);
    for (int t = threadIdx.x; t < g.n_tiles; t += kT) {
        const int2 o = tile_best[(int64_t)a * g.n_tiles + t];
        if (seed_better(g, o, mine)) mine = o;
    }
    const int2 best = seed_reduce(g, mine, s_red);
    if (threadIdx.x == 0) {
        seeds[a] = best;                      // bound >= 0: every angle has a block
        entries[a] = make_int2(a, best.y);
    }
}

// item = entry * s^2 + candidate; entries == NULL: entry e is block e % nblk of angle e / nblk.
// count (may be NULL): the list holds min(*count, n_entries) entries.  grid ceil(n_entries s^2 / kT)
__global__ __launch_bounds__(kT) void loc_fine_kernel(Dims g, const int2* keys, const uint8_t* F, const int2* entries,
                                                      const uint32_t* count, int64_t n_entries, int32_t* vol_out,
                                                      LocRec* partial, unsigned long long* n_cand) {
    __shared__ LocRec s_red[kT];
    const int64_t item = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t e = item >> (2 * g.shift);
    const int cand = (int)(item & ((1 << (2 * g.shift)) - 1));
    const int64_t n = count && (int64_t)*count < n_entries ? (int64_t)*count : n_entries;
    bool active = e < n;
    int a = 0, dx = 0, dy = 0;
    if (active) {
        int32_t b;
        if (entries) {
            const int2 en = entries[e];   // e < n <= the list's length
            a = en.x;
            b = en.y;
        } else {
            a = (int)(e / g.nblk);
            b = (int32_t)(e % g.nblk);
        }
        dx = -g.hx + (b % g.nbx) * g.s + (cand & (g.s - 1));
        dy = -g.hy + (b / g.nbx) * g.s + (cand >> g.shift);
        active = dx <= g.hx && dy <= g.hy;   // the last block of a row or column is clipped to the window
    }
    LocRec mine = {-1, 0, 0, 0};
    if (active) {
        const int2* kp = keys + (int64_t)a * g.n_pts;   // a < A
        const int sx = dx + g.hx, sy = dy + g.hy;       // 0 .. 2 * 32768
        int32_t sum = 0;
#pragma unroll 4
        for (int i = 0; i < g.n_pts; ++i) {
            const int2 k = kp[i];
            const int x = k.x + sx, y = k.y + sy;
            if ((unsigned)x < (unsigned)g.w && (unsigned)y < (unsigned)g.h) sum += (int32_t)F[(int64_t)y * g.w + x];
        }
        if (vol_out) vol_out[((int64_t)a * (2 * g.hy + 1) + sy) * (2 * g.hx + 1) + sx] = sum;   // sx <= 2 hx, sy <= 2 hy
        mine = LocRec{sum, a, dx, dy};
    }
    const int cnt = __syncthreads_count(active);
    const LocRec best = rec_reduce(g.ha, mine, s_red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = best;
        if (n_cand && cnt) atomicAdd(n_cand, (unsigned long long)cnt);
    }
}

// one workgroup: out = the best of partial[0 .. n) and *init (may be NULL)
__global__ __launch_bounds__(kT) void loc_reduce_kernel(const LocRec* partial, int64_t n, const LocRec* init, LocRec* out, int ha) {
    __shared__ LocRec s_red[kT];
    LocRec mine = {-1, 0, 0, 0};
    if (init && threadIdx.x == 0) mine = *init;
    for (int64_t i = threadIdx.x; i < n; i += kT)
        if (rec_better(ha, partial[i], mine)) mine = partial[i];
    const LocRec best = rec_reduce(ha, mine, s_red);
    if (threadIdx.x == 0) *out = best;
}

// entries[slot] = (angle, block) of every block with bound >= best0->score, slot < cap; *counter
// ends as the frontier's size whether or not it fit
__global__ __launch_bounds__(kT) void loc_frontier_kernel(const int32_t* vol, int64_t n_blocks, int32_t nblk, const LocRec* best0,
                                                          int2* entries, int64_t cap, uint32_t* counter) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n_blocks || vol[i] < best0->score) return;
    const uint32_t slot = atomicAdd(counter, 1u);   // n_blocks <= 2^29: no wrap
    if ((int64_t)slot < cap) entries[slot] = make_int2((int)(i / nblk), (int)(i % nblk));
}

// out->score = score(ha, 0, 0)
__global__ __launch_bounds__(kT) void loc_point_kernel(Dims g, const int2* keys, const uint8_t* F, LocRec* out) {
    __shared__ int32_t s_sum[kT];
    const int2* kp = keys + (int64_t)g.ha * g.n_pts;
    int32_t sum = 0;
    for (int i = threadIdx.x; i < g.n_pts; i += kT) {
        const int2 k = kp[i];
        const int x = k.x + g.hx, y = k.y + g.hy;
        if ((unsigned)x < (unsigned)g.w && (unsigned)y < (unsigned)g.h) sum += (int32_t)F[(int64_t)y * g.w + x];
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int st = kT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_sum[threadIdx.x] += s_sum[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = LocRec{s_sum[0], g.ha, 0, 0};
}

enum Mode { kLocalize, kBounds, kScores };

unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>((n + kT - 1) / kT, 1); }

// a request as the host sees it
struct Plan {
    int32_t cx, cy;
    int32_t A;
    int64_t n_blocks;   // A * nblk
    Dims g;
};

bool host_key(float v, double res, int32_t& k) {
    const double q = (double)v / res;
    if (!(fabs(q) < 536870912.0)) return false;
    k = (int32_t)round(q);
    return true;
}

int check_store(dpg_dpg* d, int64_t V, const float* est, const dpg_loc_params* p, const char* who) {
    if (!d || !est || !p) return fail(DPG_ERR_ARG, "%s: a NULL argument", who);
    if (is_multi(d->ctx)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    if (dpg_loc_params_check(p)) return fail(DPG_ERR_ARG, "%s: a parameter out of range", who);
    if (V <= 0) return fail(DPG_ERR_ARG, "%s: n_nodes out of range", who);
    return DPG_OK;
}

// the plan of the grid the field is taken from (dpg_grid.hip), under the localiser's parameters
int plan_grid(dpg_dpg* d, int64_t V, const float* est, const dpg_loc_params& P, GridPlan& gp) {
    dpg_grid_params g;
    dpg_grid_params_default(&g);
    g.resolution = P.resolution; g.max_cells = P.max_cells; g.margin_cells = P.margin_cells;
    return grid_plan(d, V, est, g, gp);
}

// the planned grid (cells > 0) on the device, then F from its occupancy bytes and, for shift > 0, P
// at that shift; ev[0] .. ev[1] bracket the kernels launched here and *ms_grid is the grid's own
int build_field(dpg_dpg* d, const GridPlan& gp, const dpg_loc_params& P, int shift, double* ms_grid) {
    dpg_grid_info info;
    int rc = grid_run(d, gp, true, &info);
    if (rc) return rc;
    *ms_grid = info.ms_kernels;
    DpgLoc& L = d->loc;
    const int32_t w = gp.box[2], h = gp.box[3], s = shift > 0 ? 1 << shift : 1;
    const int64_t pw = (int64_t)w + s - 1, ph = (int64_t)h + s - 1;
    for (DevEvent& e : L.ev)
        if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
    if (L.field.reserve((size_t)gp.cells) || (shift > 0 && (L.pool_tmp.reserve((size_t)(pw * h)) || L.pooled.reserve((size_t)(pw * ph)))))
        return fail(DPG_ERR_HIP, "out of device memory for a field of %lld cells", (long long)gp.cells);
    Stencil st;
    memset(&st, 0, sizeof(st));
    dpg_csm_params cp;
    dpg_csm_params_default(&cp);
    cp.resolution = (float)gp.res; cp.sigma = P.sigma; cp.kernel_radius = P.kernel_radius;
    if (dpg_csm_lut(&cp, st.lut)) return fail(DPG_ERR_ARG, "the resolution is not a positive float");
    st.R = P.kernel_radius; st.occupied_min = P.occupied_min;
    HIP_TRY(hipEventRecord(L.ev[0].e, d->s));
    loc_field_kernel<<<blocks_for(gp.cells), kT, 0, d->s>>>(d->d_occ_out.p, L.field.p, w, h, st);
    HIP_TRY(hipGetLastError());
    if (shift > 0) {
        loc_pool_kernel<true><<<blocks_for(pw * h), kT, 0, d->s>>>(L.field.p, L.pool_tmp.p, w, h, s);
        HIP_TRY(hipGetLastError());
        loc_pool_kernel<false><<<blocks_for(pw * ph), kT, 0, d->s>>>(L.pool_tmp.p, L.pooled.p, (int32_t)pw, h, s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(L.ev[1].e, d->s));
    return DPG_OK;
}

int make_plan(const dpg_loc_params& P, double res, const int32_t box[4], int64_t n_pts, const float guess[3], const char* who,
              Plan& pl) {
    if (!host_key(guess[0], res, pl.cx) || !host_key(guess[1], res, pl.cy) || !std::isfinite(guess[2]))
        return fail(DPG_ERR_ARG, "%s: the guess is not finite or its cell key is beyond 2^29", who);
    Dims& g = pl.g;
    memset(&g, 0, sizeof(g));
    g.shift = P.coarse_shift;
    g.s = 1 << P.coarse_shift;
    g.w = box[2]; g.h = box[3];
    g.pw = box[2] + g.s - 1; g.ph = box[3] + g.s - 1;
    g.hx = P.half_x; g.hy = P.half_y; g.ha = P.half_a;
    g.nbx = (2 * P.half_x + 1 + g.s - 1) / g.s;
    g.nby = (2 * P.half_y + 1 + g.s - 1) / g.s;
    pl.A = 2 * P.half_a + 1;
    const int64_t nblk = (int64_t)g.nbx * g.nby;
    pl.n_blocks = nblk * pl.A;
    if (pl.n_blocks > kVolMax || (int64_t)pl.A * n_pts > kVolMax)
        return fail(DPG_ERR_SIZE, "%s: %lld blocks and %lld keys, at most 2^29 each", who, (long long)pl.n_blocks,
                    (long long)((int64_t)pl.A * n_pts));
    g.nblk = (int32_t)nblk;
    g.n_pts = (int32_t)n_pts;
    g.tiles_x = (g.nbx + kTileX - 1) / kTileX;
    g.n_tiles = g.tiles_x * ((g.nby + kTileY - 1) / kTileY);
    return DPG_OK;
}

// What a search reads, filled by its two callers (the store's run() and dpg_fmap_localize): the field, its
// pooled form at the request's coarse_shift (F itself at shift 0), box and resolution, the search
// buffers and the stream.  built: L->ev[0] .. ev[1] bracket the kernels that made F and P for this call.
struct View {
    const uint8_t* F = nullptr;
    const uint8_t* P = nullptr;
    int32_t box[4] = {0, 0, 0, 0};
    double res = 0.0;
    int64_t cells = 0;
    DpgLoc* L = nullptr;
    hipStream_t s = nullptr;
    bool built = false;
    double ms_grid = 0.0;
};

// the request's own checks, before anything is planned or launched
int check_request(const float* cloud, int64_t n_pts, const float guess[3], const dpg_loc_params& P, Mode mode, int64_t cap,
                  const char* who) {
    if (n_pts < 0 || n_pts > (int64_t)1 << 23 || (n_pts > 0 && !cloud) || !guess)
        return fail(DPG_ERR_ARG, "%s: n_pts outside 0 .. 2^23, or a NULL argument", who);
    const int64_t Wx = 2 * (int64_t)P.half_x + 1, Wy = 2 * (int64_t)P.half_y + 1, A = 2 * (int64_t)P.half_a + 1;
    // sizes that depend on the parameters alone come first: a DPG_ERR_SIZE leaves nothing launched
    const int64_t s = (int64_t)1 << P.coarse_shift;
    const int64_t nb = A * ((Wx + s - 1) / s) * ((Wy + s - 1) / s);
    if (mode == kBounds && cap < nb) return fail(DPG_ERR_SIZE, "%s: out holds %lld bounds, the volume has %lld", who, (long long)cap, (long long)nb);
    if (mode == kScores && (A * Wx * Wy > kVolMax || cap < A * Wx * Wy))
        return fail(DPG_ERR_SIZE, "%s: out holds %lld scores, the volume has %lld (at most 2^29)", who, (long long)cap, (long long)(A * Wx * Wy));
    if ((mode != kBounds && (mode == kScores ? nb : std::min<int64_t>(nb, P.max_refine_blocks)) * s * s > kItemMax))
        return fail(DPG_ERR_SIZE, "%s: more than 2^36 candidates to score in one launch", who);
    return DPG_OK;
}

int search(const View& v, const float* cloud, int64_t n_pts, const float guess[3], const dpg_loc_params& P, Mode mode,
           dpg_loc_result* result, int32_t* out, const char* who);

// the whole call on a store; out: the bound volume (kBounds) or the score volume (kScores)
int run(dpg_dpg* d, int64_t V, const float* est, const float* cloud, int64_t n_pts, const float guess[3],
        const dpg_loc_params* p, Mode mode, dpg_loc_result* result, int32_t* out, int64_t cap, const char* who) {
    int rc = check_store(d, V, est, p, who);
    if (rc) return rc;
    const dpg_loc_params P = *p;
    if ((rc = check_request(cloud, n_pts, guess, P, mode, cap, who))) return rc;
    GridPlan gp;
    View v;
    if ((rc = plan_grid(d, V, est, P, gp)) || (gp.cells > 0 && (rc = build_field(d, gp, P, P.coarse_shift, &v.ms_grid)))) return rc;
    v.F = d->loc.field.p;
    v.P = P.coarse_shift > 0 ? d->loc.pooled.p : d->loc.field.p;
    memcpy(v.box, gp.box, sizeof(v.box));
    v.res = gp.res;
    v.cells = gp.cells;
    v.L = &d->loc;
    v.s = d->s;
    v.built = gp.cells > 0;
    return search(v, cloud, n_pts, guess, P, mode, result, out, who);
}

// the search of one request over a view
int search(const View& v, const float* cloud, int64_t n_pts, const float guess[3], const dpg_loc_params& P, Mode mode,
           dpg_loc_result* result, int32_t* out, const char* who) {
    int rc;
    const int64_t Wx = 2 * (int64_t)P.half_x + 1, Wy = 2 * (int64_t)P.half_y + 1, A = 2 * (int64_t)P.half_a + 1;
    const int32_t* box = v.box;
    const double res = v.res;
    Plan pl;
    if ((rc = make_plan(P, res, box, n_pts, guess, who, pl))) return rc;
    const Dims& g = pl.g;
    std::vector<float> rot((size_t)(2 * A));
    dpg_loc_rotations(guess[2], &P, rot.data());

    dpg_loc_result r;
    memset(&r, 0, sizeof(r));
    memcpy(r.box, box, sizeof(r.box));
    r.n_pts = (int32_t)n_pts;
    r.n_seeds = (int32_t)A;
    r.n_blocks = pl.n_blocks;
    LocRec win = {0, P.half_a, 0, 0};   // the winner of an all-zero volume
    if (v.cells == 0) {
        // no active node, no field: every bound and score is 0 and nothing is launched
        if (mode == kBounds) memset(out, 0, sizeof(int32_t) * (size_t)pl.n_blocks);
        if (mode == kScores) memset(out, 0, sizeof(int32_t) * (size_t)(A * Wx * Wy));
        if (mode != kLocalize) return DPG_OK;
        r.status = DPG_LOC_NO_OVERLAP;
    } else {
        DpgLoc& L = *v.L;
        hipStream_t s = v.s;
        for (DevEvent& e : L.ev)
            if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
        if (!v.built) HIP_TRY(hipEventRecord(L.ev[1].e, s));   // ms_bound starts here when no field precedes it
        const int64_t cap_f = std::min<int64_t>(P.max_refine_blocks, pl.n_blocks);
        const int64_t items_seed = A << (2 * g.shift), items_front = cap_f << (2 * g.shift);
        const int64_t items_all = pl.n_blocks << (2 * g.shift);
        const int64_t n_part = mode == kScores ? blocks_for(items_all) : mode == kLocalize ? blocks_for(items_seed) + blocks_for(items_front) : 1;
        const int64_t n_vol = mode == kScores ? std::max<int64_t>(pl.n_blocks, A * Wx * Wy) : pl.n_blocks;
        if (L.rot.reserve((size_t)(2 * A)) || L.cloud.reserve((size_t)(2 * n_pts)) || L.keys.reserve((size_t)(A * n_pts)) ||
            L.vol.reserve((size_t)n_vol) || L.tile_best.reserve((size_t)(A * g.n_tiles)) || L.seeds.reserve((size_t)A) ||
            L.entries.reserve((size_t)(A + cap_f)) || L.partial.reserve((size_t)n_part) || L.rec.reserve(4) ||
            L.counter.reserve(4))
            return fail(DPG_ERR_HIP, "%s: out of device memory for %lld blocks", who, (long long)pl.n_blocks);
        HIP_TRY(hipMemcpyAsync(L.rot.p, rot.data(), sizeof(float) * 2 * A, hipMemcpyHostToDevice, s));
        if (n_pts > 0) HIP_TRY(hipMemcpyAsync(L.cloud.p, cloud, sizeof(float) * 2 * n_pts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(L.counter.p, 0, sizeof(uint32_t) * 4, s));
        const uint8_t* Pd = v.P;
        const int64_t ox = (int64_t)pl.cx - P.half_x - box[0], oy = (int64_t)pl.cy - P.half_y - box[1];
        loc_keys_kernel<<<dim3(blocks_for(n_pts), (unsigned)A), kT, 0, s>>>(reinterpret_cast<const float2*>(L.cloud.p), L.rot.p,
                                                                          L.keys.p, g.n_pts, res, ox, oy);
        HIP_TRY(hipGetLastError());
        if (mode == kScores) {
            loc_fine_kernel<<<blocks_for(items_all), kT, 0, s>>>(g, L.keys.p, v.F, nullptr, nullptr, pl.n_blocks, L.vol.p,
                                                               L.partial.p, nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(out, L.vol.p, sizeof(int32_t) * (size_t)(A * Wx * Wy), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return DPG_OK;
        }
        loc_bound_kernel<<<dim3((unsigned)g.n_tiles, (unsigned)A), kT, 0, s>>>(g, L.keys.p, Pd, L.vol.p, L.tile_best.p);
        HIP_TRY(hipGetLastError());
        if (mode == kBounds) {
            HIP_TRY(hipMemcpyAsync(out, L.vol.p, sizeof(int32_t) * (size_t)pl.n_blocks, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return DPG_OK;
        }
        loc_seed_kernel<<<(unsigned)A, kT, 0, s>>>(g, L.tile_best.p, L.seeds.p, L.entries.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(L.ev[2].e, s));
        // counter words: [0] the frontier's size, [2..3] one 64-bit count of scored candidates
        unsigned long long* n_cand = reinterpret_cast<unsigned long long*>(L.counter.p + 2);
        const unsigned nb_seed = blocks_for(items_seed), nb_front = blocks_for(items_front);
        loc_fine_kernel<<<nb_seed, kT, 0, s>>>(g, L.keys.p, v.F, L.entries.p, nullptr, A, nullptr, L.partial.p, n_cand);
        HIP_TRY(hipGetLastError());
        loc_reduce_kernel<<<1, kT, 0, s>>>(L.partial.p, nb_seed, nullptr, L.rec.p, P.half_a);
        HIP_TRY(hipGetLastError());
        uint32_t cnt_seed[4], cnt_all[4];
        HIP_TRY(hipMemcpyAsync(cnt_seed, L.counter.p, sizeof(cnt_seed), hipMemcpyDeviceToHost, s));
        loc_frontier_kernel<<<blocks_for(pl.n_blocks), kT, 0, s>>>(L.vol.p, pl.n_blocks, g.nblk, L.rec.p, L.entries.p + A, cap_f,
                                                                  L.counter.p);
        HIP_TRY(hipGetLastError());
        loc_fine_kernel<<<nb_front, kT, 0, s>>>(g, L.keys.p, v.F, L.entries.p + A, L.counter.p, cap_f, nullptr,
                                              L.partial.p + nb_seed, n_cand);
        HIP_TRY(hipGetLastError());
        loc_reduce_kernel<<<1, kT, 0, s>>>(L.partial.p + nb_seed, nb_front, L.rec.p, L.rec.p + 1, P.half_a);
        HIP_TRY(hipGetLastError());
        loc_point_kernel<<<1, kT, 0, s>>>(g, L.keys.p, v.F, L.rec.p + 2);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(L.ev[3].e, s));
        LocRec rec[3];
        std::vector<int2> seeds((size_t)A);
        HIP_TRY(hipMemcpyAsync(rec, L.rec.p, sizeof(rec), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(cnt_all, L.counter.p, sizeof(cnt_all), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(seeds.data(), L.seeds.p, sizeof(int2) * A, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int32_t seed_max = 0;
        for (const int2& sd : seeds) seed_max = std::max(seed_max, sd.x);
        const int64_t n_front = (int64_t)cnt_all[0];
        const bool overflow = n_front > cap_f;
        win = overflow ? rec[0] : rec[1];
        r.score_at_guess = rec[2].score;
        r.n_frontier = n_front;
        uint64_t c_seed, c_all;
        memcpy(&c_seed, cnt_seed + 2, 8);
        memcpy(&c_all, cnt_all + 2, 8);
        r.n_refined_candidates = (int64_t)(overflow ? c_seed : c_all);
        if (win.score == 0 && (seed_max == 0 || !overflow)) r.status = DPG_LOC_NO_OVERLAP;
        else r.status = overflow ? DPG_LOC_UNPROVEN : DPG_LOC_OK;
        float ms[3] = {0.f, 0.f, 0.f};
        if (v.built) (void)hipEventElapsedTime(&ms[0], L.ev[0].e, L.ev[1].e);
        (void)hipEventElapsedTime(&ms[1], L.ev[1].e, L.ev[2].e);
        (void)hipEventElapsedTime(&ms[2], L.ev[2].e, L.ev[3].e);
        r.ms_field = v.ms_grid + ms[0];   // 0 when this call built nothing
        r.ms_bound = ms[1];
        r.ms_fine = ms[2];
        r.ms_kernels = r.ms_field + r.ms_bound + r.ms_fine;
    }
    r.score = win.score;
    r.best_a = win.a;
    r.best_dx = win.dx;
    r.best_dy = win.dy;
    r.pose[0] = (float)((double)((int64_t)pl.cx + win.dx) * res);
    r.pose[1] = (float)((double)((int64_t)pl.cy + win.dy) * res);
    r.pose[2] = (float)((double)guess[2] + (double)(win.a - P.half_a) * (double)P.angle_step);
    r.rot[0] = rot[(size_t)(2 * win.a)];
    r.rot[1] = rot[(size_t)(2 * win.a + 1)];
    *result = r;
    return DPG_OK;
}

// ---- the frozen map (struct dpg_fmap, dpg_dpg.h) ----
constexpr int64_t kFmapCells = (int64_t)1 << 25;   // the grid's max_cells ceiling (dpg_loc_params_check)

// an adopted map with F allocated and not yet written, or NULL with the thread's error set
dpg_fmap* fmap_new(dpg_ctx* ctx, const int32_t box[4], double res, float sigma, int32_t kernel_radius, int32_t occupied_min,
                   const char* who) {
    if (!ctx || !box) { fail(DPG_ERR_ARG, "%s: a NULL argument", who); return nullptr; }
    if (is_multi(ctx)) { fail(DPG_ERR_STATE, "%s: a frozen map lives on a single-device context", who); return nullptr; }
    if (!(res > 0.0) || !std::isfinite(res) || box[2] < 0 || box[3] < 0 || (int64_t)box[2] * box[3] > kFmapCells) {
        fail(DPG_ERR_ARG, "%s: res must be finite and > 0, w and h >= 0 and w h <= 2^25", who);
        return nullptr;
    }
    dpg_fmap* m = new dpg_fmap();
    m->ctx = ctx; m->s = ctx->stream; m->device = ctx->device;
    memcpy(m->box, box, sizeof(m->box));
    m->res = res; m->sigma = sigma; m->kernel_radius = kernel_radius; m->occupied_min = occupied_min;
    if (hipSetDevice(m->device) != hipSuccess || m->field.reserve((size_t)m->cells())) {
        delete m;
        fail(DPG_ERR_HIP, "%s: out of device memory for a field of %lld cells", who, (long long)((int64_t)box[2] * box[3]));
        return nullptr;
    }
    dpg_ctx_adopt(ctx, m, [](void* x) { dpg_fmap_destroy(static_cast<dpg_fmap*>(x)); });
    return m;
}

// P at `shift` (1 .. 5) of a non-empty map, pooled from F at the first request and kept; *built: this
// call launched the pooling, bracketed by loc.ev[0] .. ev[1]
int fmap_pooled(dpg_fmap* m, int shift, bool* built) {
    if (shift <= 0 || m->cells() == 0 || m->have_pooled[shift]) return DPG_OK;
    DpgLoc& L = m->loc;
    const int32_t w = m->box[2], h = m->box[3], s = 1 << shift;
    const int64_t pw = (int64_t)w + s - 1, ph = (int64_t)h + s - 1;
    for (DevEvent& e : L.ev)
        if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
    if (L.pool_tmp.reserve((size_t)(pw * h)) || m->pooled[shift].reserve((size_t)(pw * ph)))
        return fail(DPG_ERR_HIP, "out of device memory for a pooled field of %lld cells", (long long)(pw * ph));
    HIP_TRY(hipEventRecord(L.ev[0].e, m->s));
    loc_pool_kernel<true><<<blocks_for(pw * h), kT, 0, m->s>>>(m->field.p, L.pool_tmp.p, w, h, s);
    HIP_TRY(hipGetLastError());
    loc_pool_kernel<false><<<blocks_for(pw * ph), kT, 0, m->s>>>(L.pool_tmp.p, m->pooled[shift].p, (int32_t)pw, h, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(L.ev[1].e, m->s));
    m->have_pooled[shift] = true;
    *built = true;
    return DPG_OK;
}

}  // namespace

extern "C" {

dpg_fmap* dpg_fmap_create(dpg_dpg* d, int64_t V, const float* est, const dpg_loc_params* p) {
    const char* who = "dpg_fmap_create";
    if (check_store(d, V, est, p, who)) return nullptr;
    GridPlan gp;
    double ms = 0.0;
    if (plan_grid(d, V, est, *p, gp) || (gp.cells > 0 && build_field(d, gp, *p, 0, &ms))) return nullptr;
    dpg_fmap* m = fmap_new(d->ctx, gp.box, gp.res, p->sigma, p->kernel_radius, p->occupied_min, who);
    if (!m) return nullptr;
    if (gp.cells > 0 && (hipMemcpyAsync(m->field.p, d->loc.field.p, (size_t)gp.cells, hipMemcpyDeviceToDevice, d->s) != hipSuccess ||
                         hipStreamSynchronize(d->s) != hipSuccess)) {
        dpg_fmap_destroy(m);
        fail(DPG_ERR_HIP, "%s: the copy of the field failed", who);
        return nullptr;
    }
    return m;
}

dpg_fmap* dpg_fmap_from_field(dpg_ctx* ctx, const uint8_t* F, const int32_t box[4], double res, float sigma,
                              int32_t kernel_radius, int32_t occupied_min) {
    const char* who = "dpg_fmap_from_field";
    dpg_fmap* m = fmap_new(ctx, box, res, sigma, kernel_radius, occupied_min, who);
    if (!m) return nullptr;
    if (m->cells() > 0) {
        if (!F) {
            dpg_fmap_destroy(m);
            fail(DPG_ERR_ARG, "%s: F is NULL", who);
            return nullptr;
        }
        if (hipMemcpyAsync(m->field.p, F, (size_t)m->cells(), hipMemcpyHostToDevice, m->s) != hipSuccess ||
            hipStreamSynchronize(m->s) != hipSuccess) {
            dpg_fmap_destroy(m);
            fail(DPG_ERR_HIP, "%s: the upload of the field failed", who);
            return nullptr;
        }
    }
    return m;
}

void dpg_fmap_destroy(dpg_fmap* m) {
    if (!m) return;
    dpg_ctx_release_child(m->ctx, m);
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->s);
    delete m;
}

int dpg_fmap_info_get(const dpg_fmap* m, dpg_fmap_info* out) {
    if (!m || !out) return fail(DPG_ERR_ARG, "dpg_fmap_info_get: a NULL argument");
    memset(out, 0, sizeof(*out));
    memcpy(out->box, m->box, sizeof(out->box));
    out->res = m->res;
    out->sigma = m->sigma;
    out->kernel_radius = m->kernel_radius;
    out->occupied_min = m->occupied_min;
    out->n_bytes = m->cells();
    return DPG_OK;
}

int dpg_fmap_fetch(dpg_fmap* m, uint8_t* out, int64_t cap) {
    if (!m || (!out && m->cells() > 0)) return fail(DPG_ERR_ARG, "dpg_fmap_fetch: a NULL argument");
    if (is_multi(m->ctx)) return fail(DPG_ERR_STATE, "dpg_fmap_fetch runs on a single-device context");
    if (cap < m->cells()) return fail(DPG_ERR_SIZE, "dpg_fmap_fetch: out holds %lld bytes, the field has %lld", (long long)cap, (long long)m->cells());
    if (m->cells() == 0) return DPG_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(out, m->field.p, (size_t)m->cells(), hipMemcpyDeviceToHost, m->s));
    HIP_TRY(hipStreamSynchronize(m->s));
    return DPG_OK;
}

int dpg_fmap_save(dpg_fmap* m, const char* path) {
    if (!m || !path) return fail(DPG_ERR_ARG, "dpg_fmap_save: a NULL argument");
    const int64_t n = m->cells();
    std::vector<uint8_t> F((size_t)n);
    int rc = dpg_fmap_fetch(m, F.data(), n);
    if (rc) return rc;
    unsigned char hdr[DPG_FMAP_HEADER_SIZE];
    memset(hdr, 0, sizeof(hdr));
    const uint32_t version = 1;
    memcpy(hdr, "DPGFMAP1", 8);
    memcpy(hdr + 8, &version, 4);
    memcpy(hdr + 12, &m->kernel_radius, 4);
    memcpy(hdr + 16, &m->occupied_min, 4);
    memcpy(hdr + 20, &m->sigma, 4);
    memcpy(hdr + 24, &m->res, 8);
    memcpy(hdr + 32, m->box, 16);
    memcpy(hdr + 48, &n, 8);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(DPG_ERR_ARG, "dpg_fmap_save: cannot open %s for writing", path);
    const bool ok = fwrite(hdr, 1, sizeof(hdr), f) == sizeof(hdr) && (n == 0 || fwrite(F.data(), 1, (size_t)n, f) == (size_t)n);
    if (fclose(f) != 0 || !ok) return fail(DPG_ERR_ARG, "dpg_fmap_save: writing %s failed", path);
    return DPG_OK;
}

dpg_fmap* dpg_fmap_load(dpg_ctx* ctx, const char* path) {
    const char* who = "dpg_fmap_load";
    if (!ctx || !path) { fail(DPG_ERR_ARG, "%s: a NULL argument", who); return nullptr; }
    if (is_multi(ctx)) { fail(DPG_ERR_STATE, "%s: a frozen map lives on a single-device context", who); return nullptr; }
    FILE* f = fopen(path, "rb");
    if (!f) { fail(DPG_ERR_ARG, "%s: cannot open %s", who, path); return nullptr; }
    unsigned char hdr[DPG_FMAP_HEADER_SIZE];
    std::vector<uint8_t> F;
    long size = -1;
    bool ok = fseek(f, 0, SEEK_END) == 0 && (size = ftell(f)) >= (long)sizeof(hdr) && fseek(f, 0, SEEK_SET) == 0 &&
              fread(hdr, 1, sizeof(hdr), f) == sizeof(hdr) && dpg_fmap_header_check(hdr, (int64_t)size) == DPG_OK;
    if (ok) {
        F.resize((size_t)size - sizeof(hdr));   // = w h <= 2^25, by the check
        ok = F.empty() || fread(F.data(), 1, F.size(), f) == F.size();
    }
    fclose(f);
    if (!ok) { fail(DPG_ERR_ARG, "%s: %s is not a frozen map file (magic, version, box, res, length or reserved bytes)", who, path); return nullptr; }
    int32_t box[4], kernel_radius, occupied_min;
    float sigma;
    double res;
    memcpy(&kernel_radius, hdr + 12, 4);
    memcpy(&occupied_min, hdr + 16, 4);
    memcpy(&sigma, hdr + 20, 4);
    memcpy(&res, hdr + 24, 8);
    memcpy(box, hdr + 32, 16);
    return dpg_fmap_from_field(ctx, F.data(), box, res, sigma, kernel_radius, occupied_min);
}

int dpg_fmap_localize(dpg_fmap* m, const float* cloud, int64_t n_pts, const float guess[3], const dpg_loc_params* p,
                      dpg_loc_result* result) {
    const char* who = "dpg_fmap_localize";
    if (!m || !p || !result) return fail(DPG_ERR_ARG, "%s: a NULL argument", who);
    if (is_multi(m->ctx)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    // the fields that describe how a field is made are not read: the map has its own
    dpg_loc_params P, D;
    dpg_loc_params_default(&D);
    P = *p;
    P.resolution = D.resolution; P.max_cells = D.max_cells; P.margin_cells = D.margin_cells;
    P.sigma = D.sigma; P.kernel_radius = D.kernel_radius; P.occupied_min = D.occupied_min;
    if (dpg_loc_params_check(&P)) return fail(DPG_ERR_ARG, "%s: a parameter out of range", who);
    int rc = check_request(cloud, n_pts, guess, P, kLocalize, 0, who);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(m->device));
    View v;
    if ((rc = fmap_pooled(m, P.coarse_shift, &v.built))) return rc;
    v.F = m->field.p;
    v.P = P.coarse_shift > 0 ? m->pooled[P.coarse_shift].p : m->field.p;
    memcpy(v.box, m->box, sizeof(v.box));
    v.res = m->res;
    v.cells = m->cells();
    v.L = &m->loc;
    v.s = m->s;
    return search(v, cloud, n_pts, guess, P, kLocalize, result, nullptr, who);
}

int dpg_map_localize(dpg_dpg* d, int64_t V, const float* est, const float* cloud, int64_t n_pts, const float guess[3],
                     const dpg_loc_params* p, dpg_loc_result* result) {
    if (!result) return fail(DPG_ERR_ARG, "dpg_map_localize: result is NULL");
    return run(d, V, est, cloud, n_pts, guess, p, kLocalize, result, nullptr, 0, "dpg_map_localize");
}

int dpg_map_localize_bounds(dpg_dpg* d, int64_t V, const float* est, const float* cloud, int64_t n_pts, const float guess[3],
                            const dpg_loc_params* p, int32_t* out, int64_t cap) {
    if (!out) return fail(DPG_ERR_ARG, "dpg_map_localize_bounds: out is NULL");
    return run(d, V, est, cloud, n_pts, guess, p, kBounds, nullptr, out, cap, "dpg_map_localize_bounds");
}

int dpg_map_localize_scores(dpg_dpg* d, int64_t V, const float* est, const float* cloud, int64_t n_pts, const float guess[3],
                            const dpg_loc_params* p, int32_t* out, int64_t cap) {
    if (!out) return fail(DPG_ERR_ARG, "dpg_map_localize_scores: out is NULL");
    return run(d, V, est, cloud, n_pts, guess, p, kScores, nullptr, out, cap, "dpg_map_localize_scores");
}

int dpg_map_field(dpg_dpg* d, int64_t V, const float* est, const dpg_loc_params* p, int32_t shift, uint8_t* out, int64_t cap,
                  int32_t box[4]) {
    int rc = check_store(d, V, est, p, "dpg_map_field");
    if (rc) return rc;
    if (shift > 5) return fail(DPG_ERR_ARG, "dpg_map_field: shift above 5");
    GridPlan gp;
    if ((rc = plan_grid(d, V, est, *p, gp))) return rc;
    if (out) {
        // the size first, from the plan, so that a small cap leaves nothing launched or written
        const int64_t s = shift > 0 ? (int64_t)1 << shift : 1;
        const int64_t n = gp.cells == 0 ? 0 : shift > 0 ? (gp.box[2] + s - 1) * (gp.box[3] + s - 1) : gp.cells;
        if (cap < n) return fail(DPG_ERR_SIZE, "dpg_map_field: out holds %lld bytes, the field has %lld", (long long)cap, (long long)n);
        if (n > 0) {
            double ms = 0.0;
            if ((rc = build_field(d, gp, *p, shift, &ms))) return rc;
            HIP_TRY(hipMemcpyAsync(out, shift > 0 ? d->loc.pooled.p : d->loc.field.p, (size_t)n, hipMemcpyDeviceToHost, d->s));
            HIP_TRY(hipStreamSynchronize(d->s));
        }
    }
    if (box) memcpy(box, gp.box, sizeof(gp.box));
    return DPG_OK;
}

}  // extern "C"
