// dpg_raster.h -- the device arithmetic every parity claim of the map side rests on, once (private,
// header-only): cell keys, beams under node frames, the LDS hash probe and the reference's ray march.
// Every fp32 expression stands as the reference writes it: build includers with -ffp-contract=off.
#ifndef DPG_RASTER_H
#define DPG_RASTER_H

#include "dpg_dpg.h"

// round((double)v / res) exactly (convertToKeyForm, :923-929): v * (1/res) is within ~2 ulp of the
// quotient, so unless its fraction lies within 1e-6 of one half it rounds to the same integer as
// the correctly rounded division; only those rare near-ties pay for the fp64 division
__device__ __forceinline__ int key_of(const DS& d, float v) {
    const double q = (double)v * d.inv_res;
    const double fl = floor(q), fr = q - fl;
    if (fabs(fr - 0.5) > 1e-6) return (int)(fr < 0.5 ? fl : fl + 1.0);
    return (int)round((double)v / d.res);
}

__device__ __forceinline__ bool cell_of(const DS& d, float x, float y, int64_t* idx) {
    const int kx = key_of(d, x);
    const int ky = key_of(d, y);
    const int ix = kx - d.box.x0, iy = ky - d.box.y0;
    if (ix < 0 || iy < 0 || ix >= d.box.w || iy >= d.box.h) return false;
    *idx = (int64_t)iy * d.box.w + ix;
    return true;
}

// round((double)v / res) when the point counts (finite, |v / res| < 2^29): dpg_csm's and dpg_loc's key
__device__ __forceinline__ bool cell_key(float x, float y, double res, int& kx, int& ky) {
    const double dx = (double)x / res, dy = (double)y / res;
    if (!(fabs(dx) < 536870912.0) || !(fabs(dy) < 536870912.0)) return false;
    kx = (int)round(dx);
    ky = (int)round(dy);
    return true;
}

// map-frame point p of a beam under the frame f: transformPoint(getPointInLaserFrame, 0, lidar pose) (:844)
__device__ __forceinline__ float2 map_point_at(const float4 f, float2 p) {
    const float ns = -f.w;
    const float rx = f.z * p.x + ns * p.y;
    const float ry = f.w * p.x + f.z * p.y;
    return make_float2(f.x + rx, f.y + ry);
}

// beam b of node v under the node's estimate
__device__ __forceinline__ float2 map_point(const DS& d, int64_t v, int64_t b) {
    return map_point_at(d.frame[2 * v], d.plaser[b]);
}

// inverseTransformPoint(q, 0, lidar pose of v) (math_utils.cc:21-35)
__device__ __forceinline__ float2 rel_lidar(const DS& d, int64_t v, float2 q) {
    const float4 f = d.frame[2 * v];
    const float4 g = d.frame[2 * v + 1];
    const float tx = q.x - f.x, ty = q.y - f.y;
    const float ns = -g.y;
    return make_float2(g.x * tx + ns * ty, g.y * tx + g.x * ty);
}

// beam of an included point: node active, sector active (:917,982; every label is included,
// NOT_YET_LABELED as STATIC -- Q8 fix)
__device__ __forceinline__ bool included(const DS& d, int64_t v, int64_t b) {
    return d.active[v] && ((d.sect[v] >> d.sector[b]) & 1u);
}

// A workgroup's LDS hash set of H keys (a power of two; 0: none), slots kEmpty at the start: up to 8 probes from
// the key's multiplicative hash.  kFresh: this call claimed *slot; kSeen: the key sat in *slot; kNoSlot: neither.
constexpr uint32_t kEmpty = 0xffffffffu;
enum Probe { kFresh, kSeen, kNoSlot };

template <int H>
__device__ __forceinline__ Probe hash_probe(uint32_t* keys, uint32_t key, uint32_t* slot) {
    if (H > 0) {
        constexpr int bits = __builtin_ctz((unsigned)(H > 1 ? H : 2));
        uint32_t h = ((key * 2654435761u) >> (32 - bits)) & (uint32_t)(H - 1);
        for (int probe = 0; probe < 8; ++probe, h = (h + 1) & (uint32_t)(H - 1)) {
            const uint32_t old = atomicCAS(&keys[h], kEmpty, key);
            if (old == kEmpty || old == key) {
                *slot = h;
                return old == key ? kSeen : kFresh;
            }
        }
    }
    return kNoSlot;
}

// getIntermediateFreeCellsInFOV (:1059-1082) from the frame's lidar to the end point m: num_bins =
// round(range / res), t += 1.0 / num_bins in float, a sample at (1 - t) f + t m while t < 1.  G lanes
// share a beam: each replays the float t chain (the reference's exact sequence) up to its contiguous
// G-th of the ~nbins + 1 steps (the last lane runs to the chain's true end), then calls sample(x, y)
template <int G, typename F>
__device__ __forceinline__ void ray_march(int lane, const float4 f, const float2 m, float range, double res, F&& sample) {
    const uint32_t nbins = (uint32_t)round((double)range / res);
    const float inc = (float)(1.0 / (double)nbins);
    const uint32_t chunk = (nbins + G) / G;
    const uint32_t s0 = (uint32_t)lane * chunk, s1 = lane == G - 1 ? 0xffffffffu : s0 + chunk;
    uint32_t step = 0;
    float t = 0.0f;
    for (; step < s0 && (double)t < 1.0; ++step) t = t + inc;
    for (; step < s1 && (double)t < 1.0; t = t + inc, ++step) {
        const float ix = (1 - t) * f.x + t * m.x;
        const float iy = (1 - t) * f.y + t * m.y;
        sample(ix, iy);
    }
}

#endif
