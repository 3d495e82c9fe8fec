// dpg_change.hip -- DPG change detection on the GPU: DpgSLAM::executeDPG (dpg_slam.cc:865-886) and
// getActiveAndDynamicMapPoints (:832-863) over the device-resident node store (dpg_dpg.h; made and
// grown by dpg_store.hip).  A call is: plan (dpg_change_plan.cpp, host), reserve, stage, launch, finish.
//
// The reference keeps one hash-map occupancy grid per node (dpg_slam.h:45-260) and merges a greedy
// submap candidate by candidate.  Here every grid that matters is one bit-plane of a single dense
// window of cells around the pose chain (only chain cells are ever queried or counted):
//   word[cell] bit 2k / 2k+1 : chain node k's grid has the cell FREE-marked / OCCUPIED-marked
//   word[cell] bit 30 / 31   : the submap has it FREE-marked / OCCUPIED-marked
// OCCUPIED wins over FREE in every grid operation of the reference (:931-956,1015-1029), so all
// marking is order-free atomicOr.  The sequential greedy submap (:646-695) reduces to "candidate c
// joins iff it is the FIRST candidate (in node order) to cover some chain cell": one atomicMin pass
// gives first[cell], a histogram per candidate the coverage curve, and the threshold stop is a
// prefix walk over the (few) candidates.  DESIGN.md §K7 has the argument in full.
// Kernels: one thread per beam, blockIdx.y = node of a short list; each is described where it stands.
// Every fp32 expression is evaluated as the reference writes it (-ffp-contract=off); node frames take
// their trig on the host from the oracle's libm.  Q8 fixes: include/dpg_slam_c.h and DESIGN.md §3.
#include <string.h>

#include <algorithm>
#include <vector>

#include "dpg_atan2f.h"
#include "dpg_raster.h"

namespace {

constexpr int kT = 256;
constexpr int32_t kInf = 0x7f7f7f7f;
constexpr uint32_t kSubFree = 1u << 30, kSubOcc = 1u << 31;

// bin of the change score relative to chain node k (:815-821); -1 outside the scan's range
__device__ __forceinline__ void score_bin(const DS& d, int k, float2 q) {
    const int64_t c = d.chain[k];
    const float4 gm = d.geom[c];
    const float2 r = rel_lidar(d, c, q);
    const float a = dpg_atan2f(r.y, r.x);   // the host libm's atan2f, bit for bit
    if (a > gm.y || a < gm.x) return;
    const float inc = (gm.y - gm.x) / (float)d.total_bins;
    const uint32_t bin = (uint16_t)((a - gm.x) / inc);
    atomicOr(&d.bins[(int64_t)k * d.bin_words + (bin >> 5)], 1u << (bin & 31));
    d.inrange[k] = 1;
}

// kG lanes share a beam (ray_march), a block covers kRB / kG adjacent beams of one scan.  Near the lidar
// those rays cross the same cells over and over (hundreds of rays per cell within a metre), so a block
// first inserts a cell into an LDS hash set and only the first insertion issues the global atomic; the
// marking is a set union, so dropping repeats is exact.
constexpr int kG = 32, kRB = 1024;   // lanes per beam; raster workgroup: kRB / kG beams
constexpr int kH = 16384;            // LDS hash slots (4 B each)

template <int MODE>
__device__ __forceinline__ void mark_cell(const DS& d, uint32_t* hset, int64_t c, bool occ, int k, uint32_t fbit,
                                          uint32_t obit) {
    const uint32_t key = ((uint32_t)c << 1) | (occ ? 1u : 0u);      // c < 2^28
    uint32_t slot;
    if (hash_probe<kH>(hset, key, &slot) == kSeen) return;
    // fire-and-forget atomics (no return value, so the wave does not wait on them); first[] of a
    // cell outside the chain grids is never read
    if (MODE == 1) atomicMin(&d.first[c], k);
    else atomicOr(&d.grid[c], occ ? obit : fbit);
}

template <int MODE>
__global__ __launch_bounds__(kRB) void raster_kernel(DS d) {
    __shared__ uint32_t hset[kH];
    __shared__ unsigned long long red[2];
    const int k = blockIdx.y;
    const int lane = threadIdx.x % kG;
    for (int q = threadIdx.x; q < kH; q += kRB) hset[q] = kEmpty;
    if (threadIdx.x == 0) { red[0] = 0; red[1] = 0; }
    __syncthreads();
    bool live = !(MODE == 2 && !d.acc[k]);
    const int kc = MODE == 0 ? d.rast[k] : k;                 // chain index (MODE 0)
    const int64_t v = MODE == 0 ? d.chain[kc] : d.cand[k];
    const int64_t i = (int64_t)blockIdx.x * (kRB / kG) + threadIdx.x / kG;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    const int64_t b = b0 + i;
    live = live && i < nb && included(d, v, b);
    const int sl = MODE == 0 ? d.slot[kc] : 0;
    const uint32_t fbit = MODE == 0 ? 1u << (2 * sl) : kSubFree;
    const uint32_t obit = MODE == 0 ? 1u << (2 * sl + 1) : kSubOcc;
    unsigned long long oob = 0, ns = 0;
    if (live) {
        // a chain node's grid sits at its chain pose (current_pass_nodes_, dpg_slam.cc:591-620)
        const float4 f = MODE == 0 ? d.cframe[2 * kc] : d.frame[2 * v];
        const float2 m = MODE == 0 ? map_point_at(f, d.plaser[b]) : map_point(d, v, b);
        int64_t c;
        if (lane == 0 && d.label[b] != DPG_LABEL_MAX_RANGE) {      // occupied end point (:993-997)
            if (cell_of(d, m.x, m.y, &c)) mark_cell<MODE>(d, hset, c, true, k, fbit, obit);
            else ++oob;
        }
        ray_march<kG>(lane, f, m, d.range[b], d.res, [&](float ix, float iy) {
            ++ns;
            if (!cell_of(d, ix, iy, &c)) { ++oob; return; }
            mark_cell<MODE>(d, hset, c, false, k, fbit, obit);
        });
    }
    if (ns) atomicAdd(&red[0], ns);
    if (oob) atomicAdd(&red[1], oob);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (red[0]) atomicAdd(&d.ctl->samples, red[0]);
        if (MODE == 0 && red[1]) atomicAdd(&d.ctl->oob, red[1]);   // chain grids must fit the window
    }
}

// per-call reset of the window and the small scratch (one launch instead of seven memsets)
__global__ __launch_bounds__(kT) void init_kernel(DS d, int64_t n_cells) {
    const int64_t stride = (int64_t)gridDim.x * kT;
    const int64_t n4 = n_cells >> 2;   // 16-byte accesses (hipMalloc buffers are 256-B aligned)
    uint4* g4 = reinterpret_cast<uint4*>(d.grid);
    int4* f4 = reinterpret_cast<int4*>(d.first);
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < n4; c += stride) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (!d.rebuild) {
            w = g4[c];
            w.x &= d.keep_mask; w.y &= d.keep_mask; w.z &= d.keep_mask; w.w &= d.keep_mask;
        }
        g4[c] = w;
        f4[c] = make_int4(kInf, kInf, kInf, kInf);
    }
    for (int64_t c = 4 * n4 + (int64_t)blockIdx.x * kT + threadIdx.x; c < n_cells; c += stride) {
        d.grid[c] = d.rebuild ? 0u : (d.grid[c] & d.keep_mask);
        d.first[c] = kInf;
    }
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < d.n_cand; k += kT) { d.cand_cnt[k] = 0; d.acc[k] = 0; }
        for (int k = threadIdx.x; k < d.n_chain * d.bin_words; k += kT) d.bins[k] = 0u;
        for (int k = threadIdx.x; k < d.n_chain; k += kT) d.inrange[k] = 0;
        if (threadIdx.x == 0) memset(d.ctl, 0, sizeof(Ctl));
    }
}

// chain cells (the uncovered set at the start) and cells per first coverer: grid-stride blocks
// with an LDS histogram (up to kHist candidates), flushed once per block
constexpr int kHist = 1024;
__global__ __launch_bounds__(kT) void hist_kernel(DS d, int64_t n_cells) {
    __shared__ int32_t h[kHist];
    __shared__ unsigned long long tot;
    const bool lds = d.n_cand <= kHist;
    for (int q = threadIdx.x; q < kHist; q += kT) h[q] = 0;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const uint32_t chain_mask = d.chain_bits;
    int in = 0;
    const int64_t stride = (int64_t)gridDim.x * kT;
    auto count = [&](uint32_t w, int32_t f) {
        if (!(w & chain_mask)) return;
        ++in;
        if (f != kInf) {
            if (lds) atomicAdd(&h[f], 1);
            else atomicAdd(&d.cand_cnt[f], 1);
        }
    };
    const int64_t n4 = n_cells >> 2;   // 16-byte loads; first[] only where a chain cell is
    const uint4* g4 = reinterpret_cast<const uint4*>(d.grid);
    const int4* f4 = reinterpret_cast<const int4*>(d.first);
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < n4; c += stride) {
        const uint4 w = g4[c];
        if (!((w.x | w.y | w.z | w.w) & chain_mask)) continue;
        const int4 f = f4[c];
        count(w.x, f.x); count(w.y, f.y); count(w.z, f.z); count(w.w, f.w);
    }
    for (int64_t c = 4 * n4 + (int64_t)blockIdx.x * kT + threadIdx.x; c < n_cells; c += stride)
        count(d.grid[c], d.first[c]);
    if (in) atomicAdd(&tot, (unsigned long long)in);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(&d.ctl->chain_cells, tot);
    if (lds)
        for (int q = threadIdx.x; q < d.n_cand; q += kT)
            if (h[q]) atomicAdd(&d.cand_cnt[q], h[q]);
}

// the greedy walk of getSubMapCoveringCurrPoseChain (:646-695) over the candidates in node order
__global__ void accept_kernel(DS d) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long total = d.ctl->chain_cells;
    unsigned long long cur = total;
    bool stop = false;
    int32_t n = 0;
    for (int k = 0; k < d.n_cand; ++k) {
        d.acc[k] = 0;
        if (stop) continue;
        if (d.cand_cnt[k] > 0) {
            d.acc[k] = 1;
            cur -= (unsigned long long)d.cand_cnt[k];
            ++n;
        }
        const double coverage = 1 - ((double)cur) / (double)total;
        if (coverage >= d.cover_thr) stop = true;
    }
    d.ctl->n_acc = n;
    d.ctl->uncovered_lo = (int32_t)(cur & 0xffffffffull);
    d.ctl->uncovered_hi = (int32_t)(cur >> 32);
}

// added points of chain node k: its occupied points whose cell the submap has FREE (:757-759)
__global__ __launch_bounds__(kT) void added_kernel(DS d) {
    const int k = blockIdx.y;
    const int64_t v = d.chain[k];
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    if (i >= nb) return;
    const int64_t b = b0 + i;
    uint8_t is_added = 0;
    if (included(d, v, b) && d.label[b] != DPG_LABEL_MAX_RANGE) {
        // the cell from the chain grid's pose; the bin score from the node's estimate (:786-800)
        const float2 m = map_point_at(d.cframe[2 * k], d.plaser[b]);
        int64_t c;
        if (cell_of(d, m.x, m.y, &c)) {
            const uint32_t w = d.grid[c];
            if ((w & kSubFree) && !(w & kSubOcc)) {
                is_added = 1;
                score_bin(d, k, d.chain_sep ? map_point(d, v, b) : m);
            }
        }
    }
    d.added[(int64_t)k * d.max_beams + i] = is_added;
}

// removed points: occupied points of submap nodes in cells chain node k has FREE (:761-763)
__global__ __launch_bounds__(kT) void removed_kernel(DS d) {
    const int j = blockIdx.y;
    if (!d.acc[j]) return;
    const int64_t v = d.cand[j];
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    if (i >= nb) return;
    const int64_t b = b0 + i;
    uint32_t mask = 0;
    if (included(d, v, b) && d.label[b] != DPG_LABEL_MAX_RANGE) {
        const float2 m = map_point(d, v, b);
        int64_t c;
        if (cell_of(d, m.x, m.y, &c)) {
            const uint32_t w = d.grid[c];
            for (int k = 0; k < d.n_chain; ++k) {
                if (((w >> (2 * d.slot[k])) & 3u) == 1u) {     // FREE in chain node k's grid
                    mask |= 1u << k;
                    score_bin(d, k, m);
                }
            }
        }
    }
    d.rmask[(int64_t)j * d.max_beams + i] = (uint16_t)mask;
}

// computeBinScoreAndCommitLabelsForNode's verdict (:802-829): |bins| / totalBins >= threshold,
// evaluated only if some changed point fell inside the scan's angle range
__global__ void commit_kernel(DS d) {
    __shared__ int32_t mask;
    if (threadIdx.x == 0) mask = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < d.n_chain; k += blockDim.x) {
        int pop = 0;
        for (int w = 0; w < d.bin_words; ++w) pop += __popc(d.bins[(int64_t)k * d.bin_words + w]);
        const int ok = d.inrange[k] && ((double)pop / (double)d.total_bins >= d.change_thr);
        d.commit[k] = ok;
        if (ok) atomicOr(&mask, 1 << k);
    }
    __syncthreads();
    if (threadIdx.x == 0) d.commit[d.n_chain] = mask;
}

__global__ __launch_bounds__(kT) void apply_added_kernel(DS d) {
    const int k = blockIdx.y;
    if (!d.commit[k]) return;
    const int64_t v = d.chain[k];
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    const bool a = i < nb && d.added[(int64_t)k * d.max_beams + i];
    if (a) d.label[b0 + i] = DPG_LABEL_ADDED;
    const int cnt = __syncthreads_count(a);
    if (threadIdx.x == 0 && cnt) atomicAdd(&d.ctl->n_added, (unsigned long long)cnt);
}

// setPointLabel(REMOVED) on the point's own node (Q8 fix of :739): label + sector off
__global__ __launch_bounds__(kT) void apply_removed_kernel(DS d) {
    const int j = blockIdx.y;
    if (!d.acc[j]) return;
    const int64_t v = d.cand[j];
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    if (i >= nb) return;
    if (!(d.rmask[(int64_t)j * d.max_beams + i] & (uint32_t)d.commit[d.n_chain])) return;
    const int64_t b = b0 + i;
    d.label[b] = DPG_LABEL_REMOVED;
    const uint32_t bit = 1u << d.sector[b];
    const uint32_t old = atomicAnd(&d.sect[v], ~bit);
    if (old & bit) atomicAdd(&d.ctl->sect_off, 1ull);
    const unsigned long long slot = atomicAdd(&d.ctl->n_removed, 1ull);
    d.removed_xy[slot] = map_point(d, v, b);
}

// DpgNode::deactivateIntersectingSectors for every past node (dpg_node.cc:28-96), Q8 fix: a point
// in an already inactive sector is skipped (continue) instead of ending the loop (break)
__global__ __launch_bounds__(kT) void deactivate_kernel(DS d) {
    const int64_t v = blockIdx.x;
    if (!d.active[v]) return;
    const int64_t n_removed = (int64_t)d.ctl->n_removed;   // written by apply_removed_kernel
    __shared__ uint32_t mask;
    const uint32_t m0 = d.sect[v];
    if (threadIdx.x == 0) mask = m0;
    __syncthreads();
    const float4 gm = d.geom[v];                 // amin, amax, rmax, angle_inc
    const float sector_size = (gm.y - gm.x) / (float)d.num_sectors;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    for (int64_t q = threadIdx.x; q < n_removed; q += kT) {
        const float2 r = rel_lidar(d, v, d.removed_xy[q]);
        const float norm = __fsqrt_rn(r.x * r.x + r.y * r.y);
        if (norm > gm.z) continue;
        const float a = dpg_atan2f(r.y, r.x);   // the host libm's atan2f, bit for bit
        if (a > gm.y || a < gm.x) continue;
        const uint32_t s = (uint8_t)((a - gm.x) / sector_size);
        if ((int)s >= d.num_sectors || !((mask >> s) & 1u)) continue;
        const float approx = (a - gm.x) / gm.w;
        int64_t fl = (int64_t)floorf(approx);
        fl = fl < 0 ? 0 : (fl > nb - 1 ? nb - 1 : fl);   // bounds guard (the reference indexes unchecked)
        float fov = d.range[b0 + fl];
        if (fl < nb - 1) fov = fminf(fov, d.range[b0 + fl + 1]);
        if (fov > norm) atomicAnd(&mask, ~(1u << s));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m = mask;
        d.sect[v] = m;
        const int off = __popc(m0 & ~m);
        if (off) atomicAdd(&d.ctl->sect_off, (unsigned long long)off);
        const uint32_t full = (1u << d.num_sectors) - 1u;
        if (d.min_pct > ((float)__popc(m & full)) / (float)d.num_sectors) {
            d.active[v] = 0;
            atomicAdd(&d.ctl->nodes_off, 1ull);
        }
    }
}

// getActiveAndDynamicMapPoints: per node, the four category flags of each beam packed as 16-bit
// lanes of a u64, scanned over the block so each list keeps node/beam order
__device__ __forceinline__ uint64_t categories(const DS& d, int64_t v, int64_t b) {
    const uint8_t l = d.label[b];
    if (l == DPG_LABEL_NOT_YET_LABELED || l == DPG_LABEL_MAX_RANGE) return 0;
    uint64_t f = 0;
    if (d.active[v] && ((d.sect[v] >> d.sector[b]) & 1u)) {
        if (l == DPG_LABEL_STATIC) f |= 1ull;
        else if (l == DPG_LABEL_ADDED) f |= 1ull << 16;
    }
    if (l == DPG_LABEL_ADDED) f |= 1ull << 48;
    else if (l == DPG_LABEL_REMOVED) f |= 1ull << 32;
    return f;
}

template <bool WRITE>
__global__ __launch_bounds__(kT) void map_lists_kernel(DS d, int64_t* counts /*[V][4]*/, const int64_t* base /*[4]*/,
                                                       float2* out, int64_t cap) {
    const int64_t v = blockIdx.x;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    __shared__ uint64_t scan[kT];
    int64_t run[4] = {0, 0, 0, 0};
    if (WRITE)
        for (int l = 0; l < 4; ++l) run[l] = base[l] + counts[4 * v + l];
    for (int64_t i0 = 0; i0 < nb; i0 += kT) {
        const int64_t i = i0 + threadIdx.x;
        const uint64_t f = i < nb ? categories(d, v, b0 + i) : 0;
        scan[threadIdx.x] = f;
        __syncthreads();
        for (int s = 1; s < kT; s <<= 1) {     // inclusive Hillis-Steele over the packed lanes
            const uint64_t add = threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        const uint64_t incl = scan[threadIdx.x], tot = scan[kT - 1];
        if (WRITE && f) {
            const float2 m = map_point(d, v, b0 + i);
            const uint64_t excl = incl - f;
            for (int l = 0; l < 4; ++l) {
                if ((f >> (16 * l)) & 0xffff) {
                    const int64_t pos = run[l] + (int64_t)((excl >> (16 * l)) & 0xffff);
                    if (pos < cap) out[pos] = m;
                }
            }
        }
        for (int l = 0; l < 4; ++l) run[l] += (int64_t)((tot >> (16 * l)) & 0xffff);
        __syncthreads();
    }
    if (!WRITE && threadIdx.x == 0)
        for (int l = 0; l < 4; ++l) counts[4 * v + l] = run[l];
}

// the window (contents dropped only when the plan rebuilds it) and the per-call scratch; a failure
// leaves no kept window, since a buffer of it may be gone
int reserve_call(dpg_dpg* d, const ChangePlan& pl) {
    const size_t cells = (size_t)pl.win.w * pl.win.h, nc = std::max<size_t>(pl.cand.size(), 1), n_chain = (size_t)pl.n_chain;
    bool bad = d->d_ctl.reserve(1) || d->d_grid.reserve(cells) || d->d_first.reserve(cells);
    if (!bad && n_chain) {
        const size_t stage = (size_t)kStageCand + pl.cand.size();
        if (d->h_stage.cap < stage) bad = d->h_stage.reserve((size_t)kStageCand + std::max<size_t>(2 * pl.cand.size(), 256));
        bad = bad || d->d_stage.reserve(d->h_stage.cap) || d->d_cand_cnt.reserve(nc) || d->d_acc.reserve(nc) ||
              d->d_bins.reserve(n_chain * ((d->p.num_bins_for_change_detection + 2 + 31) / 32)) ||
              d->d_inrange.reserve(n_chain) || d->d_commit.reserve(n_chain + 1) || d->d_added.reserve(n_chain * d->max_beams) ||
              d->d_rmask.reserve(nc * d->max_beams) || d->d_removed.reserve(nc * d->max_beams);
    }
    if (!bad) return DPG_OK;
    d->kept.win_valid = false;
    return fail(DPG_ERR_HIP, "hipMalloc(change-detection window and scratch) failed");
}

// the staging block (kStage*, dpg_dpg.h) to the device and the kernels, between the two events
int stage_launch(dpg_dpg* d, const ChangePlan& pl, int64_t n_past) {
    hipStream_t s = d->s;
    HIP_TRY(hipEventRecord(d->ev[0].e, s));
    DS ds = make_ds(d);
    if (pl.n_chain > 0) {
        const unsigned nc = (unsigned)pl.cand.size(), chain_n = (unsigned)pl.n_chain;
        const int64_t cells = (int64_t)pl.win.w * pl.win.h;
        int32_t* hs = d->h_stage.p;   // the previous call ended with a stream synchronisation
        memcpy(hs + kStageChain, pl.chain, sizeof(int32_t) * chain_n);
        memcpy(hs + kStageSlot, pl.slot, sizeof(int32_t) * chain_n);
        memcpy(hs + kStageRast, pl.rast, sizeof(int32_t) * pl.n_rast);
        memcpy(hs + kStageFrames, pl.cframe, sizeof(float) * 8 * chain_n);
        if (nc) memcpy(hs + kStageCand, pl.cand.data(), sizeof(int32_t) * nc);
        HIP_TRY(hipMemcpyAsync(d->d_stage.p, hs, sizeof(int32_t) * (kStageCand + nc), hipMemcpyHostToDevice, s));
        ds.n_chain = pl.n_chain; ds.n_cand = (int32_t)nc; ds.box = pl.win; ds.rebuild = pl.reuse ? 0 : 1;
        ds.chain_bits = pl.chain_bits; ds.chain_sep = pl.chain_sep; ds.keep_mask = pl.keep_mask;
        const unsigned gx = (unsigned)((d->max_beams + kT - 1) / kT);
        const unsigned gr = (unsigned)((d->max_beams + kRB / kG - 1) / (kRB / kG));
        init_kernel<<<(unsigned)std::min<int64_t>((cells + kT - 1) / kT, 2048), kT, 0, s>>>(ds, cells);
        if (pl.n_rast) raster_kernel<0><<<dim3(gr, (unsigned)pl.n_rast), kRB, 0, s>>>(ds);
        if (nc) raster_kernel<1><<<dim3(gr, nc), kRB, 0, s>>>(ds);
        hist_kernel<<<(unsigned)std::min<int64_t>((cells + kT - 1) / kT, 1024), kT, 0, s>>>(ds, cells);
        accept_kernel<<<1, 64, 0, s>>>(ds);
        if (nc) raster_kernel<2><<<dim3(gr, nc), kRB, 0, s>>>(ds);
        added_kernel<<<dim3(gx, chain_n), kT, 0, s>>>(ds);
        if (nc) removed_kernel<<<dim3(gx, nc), kT, 0, s>>>(ds);
        commit_kernel<<<1, 64, 0, s>>>(ds);
        apply_added_kernel<<<dim3(gx, chain_n), kT, 0, s>>>(ds);
        if (nc) apply_removed_kernel<<<dim3(gx, nc), kT, 0, s>>>(ds);
    } else {   // no pose chain: only the sector/node update of the (empty) removed set runs
        HIP_TRY(hipMemsetAsync(d->d_ctl.p, 0, sizeof(Ctl), s));
    }
    // every active past node re-checks its active-sector fraction, removed points or not (dpg_node.cc:93-95)
    if (n_past > 0) deactivate_kernel<<<(unsigned)n_past, kT, 0, s>>>(ds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d->ev[1].e, s));
    return DPG_OK;
}

// read back the counters and the node activity of one dpg_execute_dpg (one synchronisation)
int finish_call(dpg_dpg* d, int64_t V, int64_t chain_n, double t0, dpg_change_stats* st) {
    hipStream_t s = d->s;
    HIP_TRY(hipMemcpyAsync(d->h_ctl.p, d->d_ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    uint32_t* act = d->h_act.p;
    HIP_TRY(hipMemcpyAsync(act, d->d_active.p, sizeof(uint32_t) * V, hipMemcpyDeviceToHost, s));
    int32_t* cm = d->h_commit.p;
    if (chain_n) HIP_TRY(hipMemcpyAsync(cm, d->d_commit.p, sizeof(int32_t) * (chain_n + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t v = 0; v < V; ++v) d->active_h[(size_t)v] = act[(size_t)v] ? 1 : 0;
    const Ctl& c = *d->h_ctl.p;
    if (c.oob) return fail(DPG_ERR_STATE, "a pose-chain ray left the change-detection window");
    st->n_submap_nodes = c.n_acc; st->n_chain_cells = (int64_t)c.chain_cells; st->n_samples = (int64_t)c.samples;
    st->n_uncovered = (int64_t)(((uint64_t)(uint32_t)c.uncovered_hi << 32) | (uint32_t)c.uncovered_lo);
    st->n_added = (int64_t)c.n_added; st->n_removed = (int64_t)c.n_removed;
    st->n_sectors_deactivated = (int64_t)c.sect_off; st->n_nodes_deactivated = (int64_t)c.nodes_off;
    for (int64_t k = 0; k < chain_n; ++k) st->n_committed += cm[(size_t)k] != 0;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, d->ev[0].e, d->ev[1].e);
    st->ms_kernels = ms;
    st->ms_total = now_ms() - t0;
    return DPG_OK;
}

}  // namespace

extern "C" {

int dpg_execute_dpg(dpg_dpg* d, int64_t V, int64_t cur_len, const float* est, dpg_change_stats* st) {
    return dpg_execute_dpg_chain(d, V, cur_len, est, nullptr, st);
}

int dpg_execute_dpg_chain(dpg_dpg* d, int64_t V, int64_t cur_len, const float* est, const float* chain_poses,
                          dpg_change_stats* st) {
    if (!d || !est || V <= 0 || V > d->V || cur_len < 0 || cur_len > V) return fail(DPG_ERR_ARG, "bad arguments");
    const double t0 = now_ms();
    dpg_change_stats local;
    if (!st) st = &local;
    memset(st, 0, sizeof(*st));
    ChangePlan pl;
    int rc = dpg_change_plan(d->p, V, cur_len, est, chain_poses, d->active_h.data(), d->rmax_beam.data(), d->kept, pl);
    st->n_chain = pl.n_chain;
    st->n_candidates = (int64_t)pl.cand.size();
    if (rc == DPG_ERR_ARG) return fail(rc, "non-finite pose in the pose chain");
    if (rc) return fail(rc, "change-detection window exceeds 2^28 cells");
    st->grid_cells = (int64_t)pl.win.w * pl.win.h;
    HIP_TRY(hipSetDevice(d->device));
    if ((rc = upload_frames(d, V, est, true)) || (rc = reserve_call(d, pl))) return rc;
    d->kept = pl.kept;
    if ((rc = stage_launch(d, pl, V - cur_len))) return rc;
    return finish_call(d, V, pl.n_chain, t0, st);
}

int64_t dpg_active_dynamic_points(dpg_dpg* d, int64_t V, const float* est, float* out, int64_t cap, int64_t counts[4]) {
    if (!d || !est || V <= 0 || V > d->V || !counts) return fail(DPG_ERR_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = d->s;
    int rc = upload_frames(d, V, est);
    if (rc) return rc;
    if (d->d_counts.reserve((size_t)(4 * V)) || d->d_base.reserve(4))
        return fail(DPG_ERR_HIP, "hipMalloc(map lists) failed");
    DS ds = make_ds(d);
    map_lists_kernel<false><<<(unsigned)V, kT, 0, s>>>(ds, d->d_counts.p, nullptr, nullptr, 0);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> cnt((size_t)(4 * V));
    HIP_TRY(hipMemcpyAsync(cnt.data(), d->d_counts.p, sizeof(int64_t) * 4 * V, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // per-node exclusive offsets inside each list, then list bases
    int64_t tot[4] = {0, 0, 0, 0};
    for (int64_t v = 0; v < V; ++v)
        for (int l = 0; l < 4; ++l) { const int64_t c = cnt[(size_t)(4 * v + l)]; cnt[(size_t)(4 * v + l)] = tot[l]; tot[l] += c; }
    int64_t base[4], total = 0;
    for (int l = 0; l < 4; ++l) { base[l] = total; total += tot[l]; counts[l] = tot[l]; }
    if (!out || cap <= 0 || total == 0) return total;
    if (d->d_map_out.reserve((size_t)std::min(cap, total))) return fail(DPG_ERR_HIP, "hipMalloc(map out) failed");
    HIP_TRY(hipMemcpyAsync(d->d_counts.p, cnt.data(), sizeof(int64_t) * 4 * V, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_base.p, base, sizeof(base), hipMemcpyHostToDevice, s));
    map_lists_kernel<true><<<(unsigned)V, kT, 0, s>>>(ds, d->d_counts.p, d->d_base.p, d->d_map_out.p, std::min(cap, total));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d->d_map_out.p, sizeof(float2) * std::min(cap, total), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return total;
}

}  // extern "C"
