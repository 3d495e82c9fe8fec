// dpg_verify.hip -- loop-closure verification by free-space consistency, batched: the kernel and its
// extern "C" entry points (dpg_verify_batch / _table / _kernel_ms).  The contract -- cell keys, the
// sensor key, the OCC and FREE cells of a model cloud, the two directions, the counts -- is the
// comment above dpg_verify_params in include/dpg_slam_c.h; the host halves (dpg_verify_params_check,
// dpg_verify_sensor_key, dpg_verify_lds_bytes) are plain C in dpg_host.c.  The reference has no such stage.
//
// One workgroup of kT threads per (pair, direction): grid (pairs, 2).  Direction 0 builds the
// target's table and streams the source's points through it, direction 1 the reverse.  LDS carve
// (dynamic, dpg_verify_lds_bytes), W = 2H + 1, pb = round_up_16(4 ceil(W W / 32)):
//   [0, pb)            the OCC plane, one bit per cell, bit v W + u for cell keys (u - H, v - H)
//   [pb, 2 pb)         the FREE plane, the same layout
//   [2 pb, +4096)      the keys of the current chunk of kChunk model points (int2; x = kNoKey: not valid)
//   [.., +64)          the three counters of the workgroup
// Table build: per chunk the points are keyed once into LDS; then every ray is walked by kG lanes,
// lane l taking i = l, l + kG, ... through the closed form off(d, n, i) (no lane depends on another's
// step), and every point's disc of radius R is spread, one cell per work item.  Both set bits with
// LDS atomicOr, so the planes are the union of what every writer marked whichever came first: no
// barrier between the two passes, identical bits every run, and chunks and points may come in any
// order.  The state of a cell is read as OCC bit ? 2 : FREE bit ? 1 : 0.
// Counting: per-thread integer counters over the moving cloud, a wave fold by shuffles, then one LDS
// atomicAdd per wave and counter; integer sums, exact in any order.  One thread stores the four
// counts of its (pair, direction); the host assembles the record and its status.
// Every loop is bounded by the validated parameters and the pair's point counts; no workgroup waits
// for another; there are no global atomics.

#include <limits.h>
#include <math.h>
#include <string.h>

#include "dpg_raster.h"   // cell_key

namespace {

constexpr int kT = 256;          // threads per workgroup
constexpr int kChunk = 512;      // model points per LDS chunk
constexpr int kG = 8;            // lanes per ray
constexpr int kScalBytes = 64;
constexpr int kNoKey = INT_MIN;  // keys[j].x of a point that does not count (a valid key is within +-2^29)
static_assert(kChunk * 8 + kScalBytes == DPG_VERIFY_LDS_FIXED, "the header's LDS formula");
static_assert(kT % 64 == 0 && kT % kG == 0 && 64 % kG == 0, "whole waves, whole ray groups inside a wave");

struct VerifyArgs {
    const float2* ds;               // the store's downsampled clouds
    const dpg_verify_pair* pairs;   // [grid.x]
    int32_t* counts;                // [grid.x][2][4]: n_pts, n_in, n_support, n_free of (pair, direction)
    uint8_t* table_out;             // diagnostic: [grid.x][2H + 1][2H + 1] state bytes, the kernel stops after the build
    double res_m;                   // (double)resolution
    int32_t H, R, ax, ay;           // ax, ay: the sensor key, |ax|, |ay| <= H
};

// The FREE cells of one ray, this lane's share: i = lane, lane + kG, ... < steps.  U is unsigned 32-bit
// when 2 (2H + 1) n fits int32, else 64-bit: 2 i minor + n <= 2 (2H) n + n < 2 (2H + 1) n.
template <typename U>
__device__ __forceinline__ void mark_ray(uint32_t* fre, int lane, int steps, int dx, int dy, int adx, int ady, int n,
                                         int ax, int ay, int H) {
    const int W = 2 * H + 1;
    const bool x_major = adx >= ady;
    const U minor = (U)(x_major ? ady : adx), nn = (U)n;
    for (int i = lane; i < steps; i += kG) {
        // along the longer axis off = floor((2 i n + n) / (2 n)) = i; along the other the division
        const int m = (int)(((U)2 * (U)i * minor + nn) / ((U)2 * nn));   // <= i <= 2H
        const int ox = x_major ? i : m, oy = x_major ? m : i;
        const int u = ax + (dx < 0 ? -ox : ox) + H, v = ay + (dy < 0 ? -oy : oy) + H;   // |.| <= 4H: no overflow
        if ((unsigned)u > (unsigned)(2 * H) || (unsigned)v > (unsigned)(2 * H)) continue;
        const int bit = v * W + u;   // in [0, W W): its word lies inside the plane
        atomicOr(&fre[bit >> 5], 1u << (bit & 31));
    }
}

__global__ __launch_bounds__(kT) void verify_kernel(VerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;
    const int dir = (int)blockIdx.y;
    const dpg_verify_pair P = a.pairs[pair];
    const int H = a.H, R = a.R, W = 2 * H + 1;
    const int pb = ((W * W + 31) / 32 * 4 + 15) / 16 * 16;   // bytes of a plane; W W <= 8 * the LDS budget
    uint32_t* occ = reinterpret_cast<uint32_t*>(smem);
    uint32_t* fre = reinterpret_cast<uint32_t*>(smem + pb);
    int2* keys = reinterpret_cast<int2*>(smem + 2 * pb);
    int32_t* s_cnt = reinterpret_cast<int32_t*>(smem + 2 * pb + kChunk * 8);
    // the model cloud (its table) and the moving cloud of this direction
    const int64_t mdl_off = dir == 0 ? P.tgt_off : P.src_off, mov_off = dir == 0 ? P.src_off : P.tgt_off;
    const int n_mdl = dir == 0 ? P.n_tgt : P.n_src, n_mov = dir == 0 ? P.n_src : P.n_tgt;

    for (int i = tid; i < 2 * pb / 4; i += kT) occ[i] = 0u;   // both planes: they are adjacent
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();

    // ---- the table of the model cloud ----
    for (int c0 = 0; c0 < n_mdl; c0 += kChunk) {
        const int nc = min(kChunk, n_mdl - c0);
        for (int j = tid; j < nc; j += kT) {   // j < kChunk
            const float2 p = a.ds[mdl_off + c0 + j];
            int kx, ky;
            if (!cell_key(p.x, p.y, a.res_m, kx, ky)) kx = kNoKey, ky = 0;
            keys[j] = make_int2(kx, ky);
        }
        __syncthreads();
        // FREE: kG lanes per ray
        for (int r = tid / kG; r < nc; r += kT / kG) {
            const int2 b = keys[r];
            if (b.x == kNoKey) continue;
            const int dx = b.x - a.ax, dy = b.y - a.ay;   // |b| <= 2^29, |a| <= H: inside int32
            const int adx = abs(dx), ady = abs(dy), n = max(adx, ady);
            const int steps = min(n, 2 * H + 1);          // the cells with i > 2H lie outside the table
            if ((int64_t)2 * (2 * H + 1) * n <= (int64_t)INT_MAX)
                mark_ray<uint32_t>(fre, tid % kG, steps, dx, dy, adx, ady, n, a.ax, a.ay, H);
            else   // a far point: rare
                mark_ray<uint64_t>(fre, tid % kG, steps, dx, dy, adx, ady, n, a.ax, a.ay, H);
        }
        // OCC: one cell of one point's (2R + 1)^2 square per work item; the corners beyond R drop out
        const int S = 2 * R + 1, S2 = S * S;
        for (int w = tid; w < nc * S2; w += kT) {   // nc S2 <= 512 * 225
            const int pt = w / S2, e = w - pt * S2;
            const int2 b = keys[pt];                // pt < nc
            if (b.x == kNoKey) continue;
            const int ox = e % S - R, oy = e / S - R;
            if (ox * ox + oy * oy > R * R) continue;
            const int u = b.x + ox + H, v = b.y + oy + H;   // |b| <= 2^29, |o| <= 7, H < 2^20: inside int32
            if ((unsigned)u > (unsigned)(2 * H) || (unsigned)v > (unsigned)(2 * H)) continue;
            const int bit = v * W + u;              // in [0, W W)
            atomicOr(&occ[bit >> 5], 1u << (bit & 31));
        }
        __syncthreads();   // the chunk's keys are done with; after the last chunk: the planes are complete
    }

    if (a.table_out) {
        uint8_t* out = a.table_out + pair * (int64_t)W * W;
        for (int i = tid; i < W * W; i += kT) {
            const uint32_t m = 1u << (i & 31);
            out[i] = (occ[i >> 5] & m) ? 2 : (fre[i >> 5] & m) ? 1 : 0;
        }
        return;
    }

    // ---- the moving cloud through the table ----
    int n_in = 0, n_sup = 0, n_fr = 0;
    for (int i = tid; i < n_mov; i += kT) {
        const float2 p = a.ds[mov_off + i];
        float qx, qy;
        if (dir == 0) {
            qx = ((P.c * p.x) - (P.s * p.y)) + P.tx;
            qy = ((P.s * p.x) + (P.c * p.y)) + P.ty;
        } else {
            const float dx = p.x - P.tx, dy = p.y - P.ty;
            qx = (P.c * dx) + (P.s * dy);
            qy = (P.c * dy) - (P.s * dx);
        }
        int kx, ky;
        if (!cell_key(qx, qy, a.res_m, kx, ky)) continue;
        const int u = kx + H, v = ky + H;   // |k| <= 2^29: inside int32
        if ((unsigned)u > (unsigned)(2 * H) || (unsigned)v > (unsigned)(2 * H)) continue;
        const int bit = v * W + u;          // in [0, W W)
        const uint32_t m = 1u << (bit & 31);
        ++n_in;
        if (occ[bit >> 5] & m) ++n_sup;
        else if (fre[bit >> 5] & m) ++n_fr;
    }
    for (int o = 32; o > 0; o >>= 1) {   // every lane of the wave is here: the loop above has ended for all
        n_in += __shfl_down(n_in, o);
        n_sup += __shfl_down(n_sup, o);
        n_fr += __shfl_down(n_fr, o);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt[0], n_in);
        atomicAdd(&s_cnt[1], n_sup);
        atomicAdd(&s_cnt[2], n_fr);
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* out = a.counts + (pair * 2 + dir) * 4;
        out[0] = n_mov;
        out[1] = s_cnt[0];
        out[2] = s_cnt[1];
        out[3] = s_cnt[2];
    }
}

int check_params(dpg_ctx* c, const dpg_verify_params* p, const char* who) {
    if (!c) return fail(DPG_ERR_ARG, "%s: ctx is NULL", who);
    if (is_multi(c)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    if (!p) return fail(DPG_ERR_ARG, "%s: params is NULL", who);
    if (dpg_verify_lds_bytes(p) < 0)
        return fail(DPG_ERR_ARG, "%s: an invalid field, a sensor outside the table, or a table above the kernel's %d bytes of LDS",
                    who, DPG_VERIFY_LDS_BUDGET);
    if (c->n_nodes <= 0) return fail(DPG_ERR_STATE, "no scans uploaded");
    return DPG_OK;
}

int fill_pair(dpg_ctx* c, int32_t t, int32_t s, const float T[6], dpg_verify_pair& q) {
    if (t < 0 || s < 0 || t >= c->n_nodes || s >= c->n_nodes) return DPG_ERR_ARG;
    memset(&q, 0, sizeof(q));
    q.tgt_off = c->ds_off[(size_t)t];
    q.src_off = c->ds_off[(size_t)s];
    const int64_t nt = c->ds_off[(size_t)t + 1] - q.tgt_off, ns = c->ds_off[(size_t)s + 1] - q.src_off;
    if (nt > INT_MAX / 256 || ns > INT_MAX / 256) return DPG_ERR_SIZE;   // the kernel's work indices stay in int32
    q.n_tgt = (int32_t)nt;
    q.n_src = (int32_t)ns;
    q.c = T[0];
    q.s = T[3];
    q.tx = T[2];
    q.ty = T[5];
    return DPG_OK;
}

// launch over `pairs` and copy back what is asked for (counts_host[pairs][2][4], or the table bytes of
// direction 0); blocks
int run(dpg_ctx* c, const dpg_verify_params& P, const std::vector<dpg_verify_pair>& pairs, int32_t* counts_host,
        uint8_t* table_host) {
    const size_t E = pairs.size();
    if (E == 0) return DPG_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t W = 2 * (size_t)P.half_cells + 1;
    if (c->ver_pairs.reserve(E) || c->ver_counts.reserve(8 * E) || c->ver_diag.reserve(table_host ? E * W * W : 0))
        return fail(DPG_ERR_HIP, "out of device memory for %zu verification pairs", E);
    if (c->ver_ev[0].ensure(hipEventDefault) || c->ver_ev[1].ensure(hipEventDefault))
        return fail(DPG_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipMemcpyAsync(c->ver_pairs.p, pairs.data(), sizeof(dpg_verify_pair) * E, hipMemcpyHostToDevice, c->stream));
    int32_t key[2];
    dpg_verify_sensor_key(&P, key);   // checked params: it succeeds
    VerifyArgs a;
    a.ds = reinterpret_cast<const float2*>(c->ds.p);
    a.pairs = c->ver_pairs.p;
    a.counts = c->ver_counts.p;
    a.table_out = table_host ? c->ver_diag.p : nullptr;
    a.res_m = (double)P.resolution;
    a.H = P.half_cells;
    a.R = P.occ_radius;
    a.ax = key[0];
    a.ay = key[1];
    const size_t lds = (size_t)dpg_verify_lds_bytes(&P);
    // more than 64 KiB of dynamic LDS: raise the kernel's limit where the runtime keeps one (its answer
    // does not matter: the launch below reports what the device refuses)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(verify_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipGetLastError();
    c->ver_timed = false;
    HIP_TRY(hipEventRecord(c->ver_ev[0].e, c->stream));
    hipLaunchKernelGGL(verify_kernel, dim3((unsigned)E, table_host ? 1u : 2u), dim3(kT), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ver_ev[1].e, c->stream));
    c->ver_timed = true;
    if (counts_host)
        HIP_TRY(hipMemcpyAsync(counts_host, c->ver_counts.p, sizeof(int32_t) * 8 * E, hipMemcpyDeviceToHost, c->stream));
    if (table_host) HIP_TRY(hipMemcpyAsync(table_host, c->ver_diag.p, E * W * W, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

}  // namespace

extern "C" {

int dpg_verify_batch(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* transforms, const dpg_verify_params* p,
                     dpg_verify_result* out, int64_t cap) {
    int rc = check_params(c, p, "dpg_verify_batch");
    if (rc) return rc;
    if (ne < 0 || ne > INT_MAX || (ne > 0 && (!edges || !transforms || !out)))
        return fail(DPG_ERR_ARG, "dpg_verify_batch: bad arguments");
    if (cap < ne) return fail(DPG_ERR_SIZE, "dpg_verify_batch: results_out holds %lld records, the batch has %lld", (long long)cap, (long long)ne);
    std::vector<dpg_verify_pair> pairs((size_t)ne);
    for (int64_t e = 0; e < ne; ++e) {
        const int32_t t = edges[2 * e], s = edges[2 * e + 1];
        rc = fill_pair(c, t, s, transforms + 6 * e, pairs[(size_t)e]);
        if (rc == DPG_ERR_ARG) return fail(rc, "edge %lld references a missing node", (long long)e);
        if (rc) return fail(rc, "edge %lld: a cloud too large", (long long)e);
    }
    std::vector<int32_t> counts((size_t)ne * 8);   // the caller's array is written only on success
    if ((rc = run(c, *p, pairs, counts.data(), nullptr))) return rc;
    for (int64_t e = 0; e < ne; ++e) {
        dpg_verify_result r;
        memset(&r, 0, sizeof(r));
        for (int d = 0; d < 2; ++d) {
            const int32_t* k = counts.data() + ((size_t)e * 2 + (size_t)d) * 4;
            r.n_pts[d] = k[0];
            r.n_in[d] = k[1];
            r.n_support[d] = k[2];
            r.n_free[d] = k[3];
        }
        r.status = r.n_in[0] == 0 || r.n_in[1] == 0 ? DPG_VERIFY_NO_OVERLAP : DPG_VERIFY_OK;
        out[e] = r;
    }
    return DPG_OK;
}

int dpg_verify_table(dpg_ctx* c, int32_t node, const dpg_verify_params* p, uint8_t* out, int64_t cap) {
    int rc = check_params(c, p, "dpg_verify_table");
    if (rc) return rc;
    if (!out) return fail(DPG_ERR_ARG, "dpg_verify_table: out is NULL");
    const int64_t W = 2 * (int64_t)p->half_cells + 1;
    if (cap < W * W) return fail(DPG_ERR_SIZE, "dpg_verify_table: out holds %lld bytes, the table has %lld", (long long)cap, (long long)(W * W));
    const float T[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    std::vector<dpg_verify_pair> pairs(1);
    if ((rc = fill_pair(c, node, node, T, pairs[0])))
        return fail(rc, "dpg_verify_table: node %d is missing or too large", node);
    return run(c, *p, pairs, nullptr, out);
}

float dpg_verify_kernel_ms(dpg_ctx* c) {
    float ms = -1.f;
    if (!c || !c->ver_timed || hipEventSynchronize(c->ver_ev[1].e) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->ver_ev[0].e, c->ver_ev[1].e) != hipSuccess) return -1.f;
    return ms;
}

}  // extern "C"
