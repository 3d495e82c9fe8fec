// dpg_grid.hip -- the occupancy grid of the active pose graph (dpg_occupancy_grid; semantics in
// include/dpg_slam_c.h; grid_plan + grid_run are the same grid left on the device for dpg_loc.hip)
// and dpg_dpg_beam_geometry.  occ_raster_kernel is the counting form of raster_kernel: the same ray
// march (dpg_raster.h), a miss per sample and a hit per end point.  A workgroup counts in an LDS
// hash table first and flushes one global atomicAdd per distinct (cell, kind) key; an add that
// finds no slot goes straight to the global counter.  All sums are integer: any order, one result.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "dpg_raster.h"

namespace {

constexpr int kT = 256;

template <int H>
__device__ __forceinline__ void occ_add(uint32_t* keys, uint32_t* cnt, int32_t* hits, int32_t* misses, int64_t c,
                                        bool hit, unsigned long long* direct) {
    const uint32_t key = ((uint32_t)c << 1) | (hit ? 1u : 0u);      // c < 2^25
    uint32_t slot;
    if (hash_probe<H>(keys, key, &slot) != kNoSlot) { atomicAdd(&cnt[slot], 1u); return; }
    atomicAdd((hit ? hits : misses) + c, 1);
    ++*direct;
}

template <int G, int RB, int H>
__global__ __launch_bounds__(RB) void occ_raster_kernel(DS d, const int32_t* nodes, int32_t blocks_per_node,
                                                        int32_t* hits, int32_t* misses, OccCtl* ctl) {
    constexpr int HS = H > 0 ? H : 1;
    __shared__ uint32_t keys[HS];
    __shared__ uint32_t cnt[HS];
    __shared__ unsigned long long red[6];
    const int64_t v = nodes[blockIdx.x / blocks_per_node];
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_node) * (RB / G) + threadIdx.x / G;
    const int64_t b0 = d.off[v], nb = d.off[v + 1] - b0;
    const int64_t b = b0 + i;
    const bool live = i < nb && included(d, v, b);
    if (!__syncthreads_or(live)) return;      // inactive node, inactive sectors or past the scan's end
    for (int q = threadIdx.x; q < HS; q += RB) { keys[q] = kEmpty; cnt[q] = 0u; }
    if (threadIdx.x < 6) red[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long ns = 0, oob = 0, nh = 0, direct = 0, flushed = 0;
    if (live) {
        const float4 f = d.frame[2 * v];
        const float2 m = map_point(d, v, b);
        const uint8_t l = d.label[b];
        int64_t c, hit_cell = -1;
        if (l != DPG_LABEL_MAX_RANGE && l != DPG_LABEL_REMOVED) {
            if (cell_of(d, m.x, m.y, &c)) {
                hit_cell = c;
                if (lane == 0) { occ_add<H>(keys, cnt, hits, misses, c, true, &direct); ++nh; }
            } else if (lane == 0) {
                ++oob;
            }
        }
        ray_march<G>(lane, f, m, d.range[b], d.res, [&](float ix, float iy) {
            ++ns;
            if (!cell_of(d, ix, iy, &c)) { ++oob; return; }
            if (c == hit_cell) return;      // the beam's own hit cell is not also a miss
            occ_add<H>(keys, cnt, hits, misses, c, false, &direct);
        });
    }
    __syncthreads();
    if (H > 0)
        for (int q = threadIdx.x; q < HS; q += RB) {
            const uint32_t key = keys[q];
            if (key == kEmpty) continue;
            atomicAdd(((key & 1u) ? hits : misses) + (key >> 1), (int32_t)cnt[q]);
            ++flushed;
        }
    if (ns) atomicAdd(&red[0], ns);
    if (oob) atomicAdd(&red[1], oob);
    if (nh) atomicAdd(&red[2], nh);
    if (direct) atomicAdd(&red[3], direct);
    if (flushed) atomicAdd(&red[4], flushed);
    if (live && lane == 0) atomicAdd(&red[5], 1ull);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (red[0]) atomicAdd(&ctl->samples, red[0]);
        if (red[1]) atomicAdd(&ctl->oob, red[1]);
        if (red[2]) atomicAdd(&ctl->hits, red[2]);
        if (red[3]) atomicAdd(&ctl->direct, red[3]);
        if (red[4]) atomicAdd(&ctl->flushed, red[4]);
        if (red[5]) atomicAdd(&ctl->beams, red[5]);
    }
}

__device__ __forceinline__ uint32_t occ_byte(int32_t h, int32_t m) {
    const int64_t n = (int64_t)h + m;
    return n == 0 ? 0xffu : (uint32_t)((200 * (int64_t)h + n) / (2 * n));
}

__device__ __forceinline__ uint32_t occ_word(int4 h, int4 m) {
    return occ_byte(h.x, m.x) | (occ_byte(h.y, m.y) << 8) | (occ_byte(h.z, m.z) << 16) | (occ_byte(h.w, m.w) << 24);
}

// hits, misses -> occupancy bytes, 16 cells per thread and one 16-byte store (the three buffers
// start on 256-B boundaries)
__global__ __launch_bounds__(kT) void occ_finalize_kernel(const int32_t* hits, const int32_t* misses, int8_t* occ,
                                                          int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kT, n16 = n >> 4;
    const int4* h4 = reinterpret_cast<const int4*>(hits);
    const int4* m4 = reinterpret_cast<const int4*>(misses);
    uint4* o4 = reinterpret_cast<uint4*>(occ);
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < n16; c += stride)
        o4[c] = make_uint4(occ_word(h4[4 * c], m4[4 * c]), occ_word(h4[4 * c + 1], m4[4 * c + 1]),
                           occ_word(h4[4 * c + 2], m4[4 * c + 2]), occ_word(h4[4 * c + 3], m4[4 * c + 3]));
    for (int64_t c = 16 * n16 + (int64_t)blockIdx.x * kT + threadIdx.x; c < n; c += stride)
        occ[c] = (int8_t)occ_byte(hits[c], misses[c]);
}

// dpg_dpg_beam_geometry: one thread per beam (its node by bisection of the offsets) and per node
__global__ __launch_bounds__(kT) void beam_geometry_kernel(DS d, int64_t V, int64_t n_beams, float2* lidar_xy,
                                                           float2* end_xy) {
    const int64_t b = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (lidar_xy && b < V) {
        const float4 f = d.frame[2 * b];
        lidar_xy[b] = make_float2(f.x, f.y);
    }
    if (!end_xy || b >= n_beams) return;
    int64_t lo = 0, hi = V;                    // off[lo] <= b < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (d.off[mid] <= b) lo = mid;
        else hi = mid;
    }
    end_xy[b] = map_point(d, lo, b);
}

// occ_raster_kernel's lane group / workgroup / LDS table slots.  Variant 0 is the product: 8 lanes per
// beam, 128 beams per 1024-thread workgroup, 8192 slots (64 KB, two workgroups per CU): a wave's time is
// the t chain of its longest beam, so time falls with the lane group until the beams overflow the table.
// The other variants give the same grid, for tools/occ_grid_probe.py (DESIGN.md K7 holds the measurements).
template <int G, int RB, int H>
void occ_launch(const DS& ds, const int32_t* nodes, int64_t n_nodes, int32_t max_beams, int32_t* hits,
                int32_t* misses, OccCtl* ctl, hipStream_t s) {
    const int32_t bpn = (max_beams + RB / G - 1) / (RB / G);
    occ_raster_kernel<G, RB, H><<<(unsigned)(n_nodes * bpn), RB, 0, s>>>(ds, nodes, bpn, hits, misses, ctl);
}

constexpr int kOccBeamsMin = 1024 / 32;   // fewest beams per workgroup among the variants (grid size bound)
typedef void (*OccLaunch)(const DS&, const int32_t*, int64_t, int32_t, int32_t*, int32_t*, OccCtl*, hipStream_t);
const OccLaunch kOccLaunch[] = {   // by dpg_grid_params.pad; 1: raster_kernel's split, 7: no table, every add global
    occ_launch<8, 1024, 8192>, occ_launch<32, 1024, 8192>, occ_launch<16, 1024, 8192>, occ_launch<8, 1024, 8192>,
    occ_launch<4, 1024, 8192>, occ_launch<8, 512, 4096>,   occ_launch<16, 512, 4096>,  occ_launch<32, 1024, 0>,
    occ_launch<8, 512, 8192>,  occ_launch<4, 512, 4096>};
constexpr int kOccVariants = sizeof(kOccLaunch) / sizeof(kOccLaunch[0]);

}  // namespace

int grid_plan(dpg_dpg* d, int64_t V, const float* est, const dpg_grid_params& p, GridPlan& g) {
    if (!d || !est || V <= 0 || V > d->V) return fail(DPG_ERR_ARG, "bad arguments");
    g.res = p.resolution == 0.0 ? d->p.occ_grid_resolution : p.resolution;
    g.variant = p.pad;
    const int64_t max_cells = p.max_cells == 0 ? (int64_t)1 << 25 : p.max_cells;
    if (!(g.res > 0.0) || !std::isfinite(g.res) || max_cells < 0 || max_cells > (int64_t)1 << 25 || p.margin_cells < 0 ||
        p.pad < 0 || p.pad >= kOccVariants)
        return fail(DPG_ERR_ARG, "grid params out of range (resolution > 0, max_cells <= 2^25, margin >= 0)");
    HIP_TRY(hipSetDevice(d->device));
    int rc = upload_frames(d, V, est, true);
    if (rc) return rc;
    // the box over the active nodes (host mirror of the activity, the cached lidar positions)
    std::vector<float> lidar((size_t)(2 * V));
    g.nodes.clear();
    for (int64_t v = 0; v < V; ++v) {
        lidar[(size_t)(2 * v)] = d->h_frames.p[8 * v];
        lidar[(size_t)(2 * v + 1)] = d->h_frames.p[8 * v + 1];
        if (d->active_h[(size_t)v]) g.nodes.push_back((int32_t)v);
    }
    rc = dpg_grid_box(lidar.data(), d->rmax_beam.data(), d->active_h.data(), V, g.res, p.margin_cells, g.box);
    if (rc == DPG_ERR_ARG) return fail(rc, "non-finite pose or range of an active node");
    if (rc) return fail(rc, "occupancy grid box exceeds the key range");
    g.cells = (int64_t)g.box[2] * g.box[3];
    if (g.cells > max_cells) return fail(DPG_ERR_SIZE, "occupancy grid box exceeds max_cells");
    return DPG_OK;
}

int grid_run(dpg_dpg* d, const GridPlan& g, bool want_occ, dpg_grid_info* info) {
    hipStream_t s = d->s;
    const int64_t n = (int64_t)g.nodes.size(), cells = g.cells, pitch = grid_pitch(cells);
    if (n * ((d->max_beams + kOccBeamsMin - 1) / kOccBeamsMin) > (int64_t)INT32_MAX)
        return fail(DPG_ERR_SIZE, "too many active scans for one launch");
    if (d->d_occ_cnt.reserve((size_t)(2 * pitch)) || d->d_occ_out.reserve((size_t)cells) ||
        d->d_occ_nodes.reserve((size_t)n) || d->d_occ_ctl.reserve(1))
        return fail(DPG_ERR_HIP, "hipMalloc(occupancy grid) failed");
    DS ds = make_ds(d);
    ds.res = g.res; ds.inv_res = 1.0 / g.res;
    ds.box = Box{g.box[0], g.box[1], g.box[2], g.box[3]};
    int32_t *dh = d->d_occ_cnt.p, *dm = d->d_occ_cnt.p + pitch;
    HIP_TRY(hipMemcpyAsync(d->d_occ_nodes.p, g.nodes.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(d->ev[0].e, s));
    HIP_TRY(hipMemsetAsync(d->d_occ_cnt.p, 0, sizeof(int32_t) * 2 * pitch, s));
    HIP_TRY(hipMemsetAsync(d->d_occ_ctl.p, 0, sizeof(OccCtl), s));
    kOccLaunch[g.variant](ds, d->d_occ_nodes.p, n, d->max_beams, dh, dm, d->d_occ_ctl.p, s);
    HIP_TRY(hipGetLastError());
    if (want_occ) {
        occ_finalize_kernel<<<(unsigned)std::min<int64_t>((cells / 16 + kT) / kT, 2048), kT, 0, s>>>(dh, dm, d->d_occ_out.p, cells);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(d->ev[1].e, s));
    OccCtl c;
    HIP_TRY(hipMemcpyAsync(&c, d->d_occ_ctl.p, sizeof(c), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info->n_beams_used = (int64_t)c.beams; info->n_hits = (int64_t)c.hits; info->n_samples = (int64_t)c.samples;
    info->n_oob = (int64_t)c.oob; info->n_direct = (int64_t)c.direct; info->n_flushed = (int64_t)c.flushed;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, d->ev[0].e, d->ev[1].e);
    info->ms_kernels = ms;
    return DPG_OK;
}

extern "C" {

int dpg_occupancy_grid(dpg_dpg* d, int64_t V, const float* est, const dpg_grid_params* gp, int32_t* hits,
                       int32_t* misses, int8_t* occ, int64_t cap, dpg_grid_info* info) {
    const double t0 = now_ms();
    GridPlan g;
    int rc = grid_plan(d, V, est, or_default(gp, dpg_grid_params_default), g);
    if (rc) return rc;
    dpg_grid_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    info->resolution = g.res;
    info->x0 = g.box[0]; info->y0 = g.box[1]; info->w = g.box[2]; info->h = g.box[3];
    info->n_nodes_used = (int64_t)g.nodes.size();
    const bool plan_only = !hits && !misses && !occ;
    if (!plan_only && cap < g.cells) return fail(DPG_ERR_SIZE, "output arrays hold fewer than w * h cells");
    if (!plan_only && g.cells > 0) {
        // the outputs are staged so that a failure of the run leaves the caller's arrays untouched
        if ((rc = grid_run(d, g, occ != nullptr, info))) return rc;
        hipStream_t s = d->s;
        const int32_t* dh = d->d_occ_cnt.p;
        if (hits) HIP_TRY(hipMemcpyAsync(hits, dh, sizeof(int32_t) * g.cells, hipMemcpyDeviceToHost, s));
        if (misses) HIP_TRY(hipMemcpyAsync(misses, dh + grid_pitch(g.cells), sizeof(int32_t) * g.cells, hipMemcpyDeviceToHost, s));
        if (occ) HIP_TRY(hipMemcpyAsync(occ, d->d_occ_out.p, (size_t)g.cells, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    info->ms_total = now_ms() - t0;
    return DPG_OK;
}

int dpg_dpg_beam_geometry(dpg_dpg* d, int64_t V, const float* est, float* lidar_xy, float* end_xy, int64_t cap_beams) {
    if (!d || !est || V <= 0 || V > d->V) return fail(DPG_ERR_ARG, "bad arguments");
    const int64_t nB = d->off[(size_t)V];
    if (end_xy && cap_beams < nB) return fail(DPG_ERR_SIZE, "end_xy holds fewer beams than the nodes have");
    if (!lidar_xy && !end_xy) return DPG_OK;
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = d->s;
    int rc = upload_frames(d, V, est);
    if (rc) return rc;
    if (d->d_geo.reserve((size_t)(V + nB))) return fail(DPG_ERR_HIP, "hipMalloc(beam geometry) failed");
    float2 *dl = d->d_geo.p, *de = d->d_geo.p + V;
    const DS ds = make_ds(d);
    const int64_t threads = std::max(V, nB);
    beam_geometry_kernel<<<(unsigned)((threads + kT - 1) / kT), kT, 0, s>>>(ds, V, nB, lidar_xy ? dl : nullptr,
                                                                            end_xy ? de : nullptr);
    HIP_TRY(hipGetLastError());
    if (lidar_xy) HIP_TRY(hipMemcpyAsync(lidar_xy, dl, sizeof(float2) * V, hipMemcpyDeviceToHost, s));
    if (end_xy) HIP_TRY(hipMemcpyAsync(end_xy, de, sizeof(float2) * nB, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DPG_OK;
}

}  // extern "C"
