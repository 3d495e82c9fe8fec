// dpg_loc_dev.h -- the device arithmetic that the map search (dpg_loc.hip) and the tracker
// (dpg_track.hip) share, once (private, header-only): the key rule of a rotated point and the
// winner's order with its LDS tree.  The contract is the comment above dpg_loc_params in
// include/dpg_slam_c.h.  Every fp32 expression stands as written there: -ffp-contract=off.
#ifndef DPG_LOC_DEV_H
#define DPG_LOC_DEV_H

#include "dpg_raster.h"

constexpr int kLocT = 256;               // threads per workgroup
constexpr int kLocChunk = 2048;          // keys per LDS chunk (16 KiB)
constexpr int kKeyNone = -(1 << 30);     // key of a point that contributes nothing: no shift brings it to an index >= -(s - 1)
constexpr int64_t kKeyLim = (int64_t)1 << 27;   // |key| beyond this reaches no cell of a box of <= 2^25 cells under any shift

// the field index of point p under (c, s) at the window's first shift: (kx + ox, ky + oy) with
// (ox, oy) = (cx - hx - x0, cy - hy - y0), or (kKeyNone, kKeyNone)
__device__ __forceinline__ int2 loc_key(float2 p, float c, float s, double res, int64_t ox, int64_t oy) {
    const float rx = (c * p.x) - (s * p.y);
    const float ry = (s * p.x) + (c * p.y);
    int2 k = make_int2(kKeyNone, kKeyNone);
    int kx, ky;
    if (cell_key(rx, ry, res, kx, ky)) {
        const int64_t ux = (int64_t)kx + ox, uy = (int64_t)ky + oy;
        if (ux >= -kKeyLim && ux <= kKeyLim && uy >= -kKeyLim && uy <= kKeyLim) k = make_int2((int)ux, (int)uy);
    }
    return k;
}

// the winner's order: higher score, then smaller |a - ha|, dx^2 + dy^2, a, dy, dx
__device__ __forceinline__ bool rec_better(int ha, const LocRec& x, const LocRec& y) {
    if (x.score != y.score) return x.score > y.score;
    if (x.score < 0) return false;
    const int ax = abs(x.a - ha), ay = abs(y.a - ha);
    if (ax != ay) return ax < ay;
    const int64_t dx = (int64_t)x.dx * x.dx + (int64_t)x.dy * x.dy, dy = (int64_t)y.dx * y.dx + (int64_t)y.dy * y.dy;
    if (dx != dy) return dx < dy;
    if (x.a != y.a) return x.a < y.a;
    if (x.dy != y.dy) return x.dy < y.dy;
    return x.dx < y.dx;
}
// the best of a workgroup of kLocT threads, field by field (the keys do not fit 64 bits)
__device__ __forceinline__ LocRec rec_reduce(int ha, LocRec mine, LocRec* sh) {
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int st = kLocT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st && rec_better(ha, sh[threadIdx.x + st], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + st];
        __syncthreads();
    }
    return sh[0];
}

#endif
