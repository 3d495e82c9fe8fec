// dpg_track.hip -- dpg_fmap_track: a batch of scans, each searched exhaustively over a small window
// of a frozen map's field, in one enqueue.  The contract is the comment above dpg_track_params in
// include/dpg_slam_c.h: the records are those of dpg_map_localize at coarse_shift 0 for the same
// window and guess (keys, score, winner's order: dpg_loc_dev.h).  The reference has no such stage.
//
// Windows this small do not amortise a key table in global memory or a bound volume, so:
//   track_scan_kernel    a workgroup = one (scan, angle): it rotates and keys the scan's points itself
//                        into LDS, a chunk of 2048 keys at a time; a thread owns the shifts
//                        tid + 256 k of the (2 half_x + 1)(2 half_y + 1) window, lanes along dx, so for
//                        one point a wave reads consecutive bytes of one row of F (through L2) and the
//                        key is one LDS broadcast read; the shifts of a thread are scored one after the
//                        other, so only a running best is kept in registers; a scan of more than one
//                        chunk is keyed again for every k (rare: a chunk holds a whole 2048-beam scan);
//                        the workgroup's best in the winner's order through an LDS tree; the
//                        thread that owns (half_a, 0, 0) writes the score at the guess
//   track_reduce_kernel  a workgroup per scan: the best of its angles
// Every loop is bounded by the validated parameters and the offsets, every index is tested against
// the box at its access, no workgroup waits for another and no result goes through an atomic.
// The host side is in stages (track_check, track_stage, track_launch, track_results: dpg_dpg.h) that
// dpg_fmap_track_refine (dpg_refine.hip) runs too, with its refinement enqueued behind the launches.

#include <math.h>
#include <string.h>

#include <cmath>

#include "dpg_loc_dev.h"

namespace {

struct TrackDims {
    int32_t w, h;          // F [h][w]
    int32_t x0, y0;
    int32_t hx, hy, ha;
    int32_t A, wx, n_shifts;   // 2 ha + 1, 2 hx + 1, (2 hx + 1)(2 hy + 1)
    double res;
};

// grid (A, B)
__global__ __launch_bounds__(kLocT) void track_scan_kernel(TrackDims g, const TrackScan* scans, const float2* cloud, const float* rot,
                                                           const uint8_t* F, LocRec* part, int32_t* at_guess) {
    __shared__ int2 s_keys[kLocChunk];
    __shared__ LocRec s_red[kLocT];
    const int tid = threadIdx.x, a = blockIdx.x;
    const int64_t b = blockIdx.y;
    const TrackScan sc = scans[b];                                   // b < B
    const float c = rot[(b * g.A + a) * 2], s = rot[(b * g.A + a) * 2 + 1];   // a < A
    const int64_t n = sc.end - sc.begin;                             // 0 .. 2^23
    const int64_t ox = (int64_t)sc.cx - g.hx - g.x0, oy = (int64_t)sc.cy - g.hy - g.y0;
    const bool one = n <= kLocChunk;
    auto fill = [&](int64_t c0, int m) {                             // m keys of the points from c0 on
        for (int i = tid; i < m; i += kLocT) s_keys[i] = loc_key(cloud[sc.begin + c0 + i], c, s, g.res, ox, oy);   // c0 + i < n
    };
    if (one) {
        fill(0, (int)n);
        __syncthreads();
    }
    LocRec mine = {-1, 0, 0, 0};
    const int at = g.hy * g.wx + g.hx;                               // the shift (0, 0)
    for (int j0 = 0; j0 < g.n_shifts; j0 += kLocT) {                 // uniform over the workgroup
        const int j = j0 + tid;
        const bool active = j < g.n_shifts;
        const int sx = j % g.wx, sy = j / g.wx;                      // 0 .. 128
        int32_t sum = 0;
        for (int64_t c0 = 0; c0 < n; c0 += kLocChunk) {
            const int m = (int)(n - c0 < kLocChunk ? n - c0 : kLocChunk);
            if (!one) {
                __syncthreads();                                     // the chunk's last readers are done
                fill(c0, m);
                __syncthreads();
            }
            if (active) {
#pragma unroll 4
                for (int i = 0; i < m; ++i) {
                    const int2 k = s_keys[i];                        // |k| <= 2^27 or kKeyNone: no overflow below
                    const int x = k.x + sx, y = k.y + sy;
                    if ((unsigned)x < (unsigned)g.w && (unsigned)y < (unsigned)g.h) sum += (int32_t)F[(int64_t)y * g.w + x];
                }
            }
        }
        if (active) {
            const LocRec r = {sum, a, sx - g.hx, sy - g.hy};
            if (rec_better(g.ha, r, mine)) mine = r;
            if (a == g.ha && j == at) at_guess[b] = sum;
        }
    }
    const LocRec best = rec_reduce(g.ha, mine, s_red);
    if (tid == 0) part[b * g.A + a] = best;
}

// grid B: recs[b] = the best of part[b][0 .. A) and the score at the guess
__global__ __launch_bounds__(kLocT) void track_reduce_kernel(TrackDims g, const LocRec* part, const int32_t* at_guess, TrackRec* recs) {
    __shared__ LocRec s_red[kLocT];
    const int64_t b = blockIdx.x;
    LocRec mine = {-1, 0, 0, 0};
    for (int a = threadIdx.x; a < g.A; a += kLocT) {
        const LocRec o = part[b * g.A + a];
        if (rec_better(g.ha, o, mine)) mine = o;
    }
    const LocRec best = rec_reduce(g.ha, mine, s_red);
    if (threadIdx.x == 0) {
        TrackRec r;
        r.win = best;
        r.score_at_guess = at_guess[b];
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        recs[b] = r;
    }
}

bool host_key(float v, double res, int32_t& k) {
    const double q = (double)v / res;
    if (!(fabs(q) < 536870912.0)) return false;
    k = (int32_t)round(q);
    return true;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

int track_check(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                const dpg_track_params* p, const void* out, const char* who) {
    if (!m || !p || !offsets || B < 0 || (B > 0 && (!guesses || !out))) return fail(DPG_ERR_ARG, "%s: a NULL argument or B < 0", who);
    if (is_multi(m->ctx)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    if (dpg_track_params_check(p)) return fail(DPG_ERR_ARG, "%s: a parameter out of range", who);
    if (B > 65535) return fail(DPG_ERR_SIZE, "%s: %lld scans, at most 65535 in a call", who, (long long)B);
    if (offsets[0] < 0) return fail(DPG_ERR_ARG, "%s: offsets[0] is negative", who);
    for (int64_t b = 0; b < B; ++b)
        if (offsets[b + 1] < offsets[b]) return fail(DPG_ERR_ARG, "%s: offsets are not monotone at scan %lld", who, (long long)b);
    for (int64_t b = 0; b < B; ++b)
        if (offsets[b + 1] - offsets[b] > (int64_t)1 << 23) return fail(DPG_ERR_SIZE, "%s: scan %lld has more than 2^23 points", who, (long long)b);
    const int64_t total = offsets[B] - offsets[0];
    if (total > (int64_t)1 << 26) return fail(DPG_ERR_SIZE, "%s: %lld points in all, at most 2^26", who, (long long)total);
    if (total > 0 && !clouds) return fail(DPG_ERR_ARG, "%s: clouds_xy is NULL", who);
    return DPG_OK;
}

int track_stage(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                const dpg_track_params* p, const char* who, TrackStage& st) {
    st.P = *p;
    st.B = B;
    st.A = 2 * (int64_t)st.P.half_a + 1;
    st.total = offsets[B] - offsets[0];
    const int64_t A = st.A;
    st.o_scan = 0;
    st.o_rot = align16(st.o_scan + sizeof(TrackScan) * (size_t)B);
    st.o_pts = align16(st.o_rot + sizeof(float) * 2 * (size_t)(A * B));
    st.n_in = align16(st.o_pts + sizeof(float) * 2 * (size_t)st.total);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->s));   // the pinned blocks of the previous call are free
    if (m->h_in.reserve(st.n_in)) return fail(DPG_ERR_HIP, "%s: out of pinned memory for %lld scans", who, (long long)B);
    st.scans = reinterpret_cast<TrackScan*>(m->h_in.p + st.o_scan);
    st.rot = reinterpret_cast<float*>(m->h_in.p + st.o_rot);
    dpg_loc_params lp;
    dpg_loc_params_default(&lp);
    lp.half_a = st.P.half_a;
    lp.angle_step = st.P.angle_step;
    for (int64_t b = 0; b < B; ++b) {
        const float* g = guesses + 3 * b;
        TrackScan& t = st.scans[b];
        memset(&t, 0, sizeof(t));
        if (!host_key(g[0], m->res, t.cx) || !host_key(g[1], m->res, t.cy) || !std::isfinite(g[2]))
            return fail(DPG_ERR_ARG, "%s: the guess of scan %lld is not finite or its cell key is beyond 2^29", who, (long long)b);
        t.begin = offsets[b] - offsets[0];
        t.end = offsets[b + 1] - offsets[0];
        dpg_loc_rotations(g[2], &lp, st.rot + 2 * A * b);
    }
    if (st.total > 0) memcpy(m->h_in.p + st.o_pts, clouds + 2 * offsets[0], sizeof(float) * 2 * (size_t)st.total);
    return DPG_OK;
}

int track_launch(dpg_fmap* m, const TrackStage& st, TrackRec* d_recs, const char* who) {
    const dpg_track_params& P = st.P;
    const int64_t A = st.A, B = st.B;
    if (m->part.reserve((size_t)(A * B)) || m->at_guess.reserve((size_t)B))
        return fail(DPG_ERR_HIP, "%s: out of device memory for %lld scans", who, (long long)B);
    TrackDims g;
    memset(&g, 0, sizeof(g));
    g.w = m->box[2]; g.h = m->box[3]; g.x0 = m->box[0]; g.y0 = m->box[1];
    g.hx = P.half_x; g.hy = P.half_y; g.ha = P.half_a;
    g.A = (int32_t)A; g.wx = 2 * P.half_x + 1; g.n_shifts = g.wx * (2 * P.half_y + 1);
    g.res = m->res;
    const TrackScan* d_scans = reinterpret_cast<const TrackScan*>(m->d_in.p + st.o_scan);
    track_scan_kernel<<<dim3((unsigned)A, (unsigned)B), kLocT, 0, m->s>>>(g, d_scans, reinterpret_cast<const float2*>(m->d_in.p + st.o_pts),
                                                                        reinterpret_cast<const float*>(m->d_in.p + st.o_rot), m->field.p,
                                                                        m->part.p, m->at_guess.p);
    HIP_TRY(hipGetLastError());
    track_reduce_kernel<<<(unsigned)B, kLocT, 0, m->s>>>(g, m->part.p, m->at_guess.p, d_recs);
    HIP_TRY(hipGetLastError());
    return DPG_OK;
}

void track_results(const dpg_fmap* m, const TrackStage& st, const float* guesses, const TrackRec* recs, dpg_track_result* out) {
    const dpg_track_params& P = st.P;
    for (int64_t b = 0; b < st.B; ++b) {
        // an empty map: every score is 0, the winner of an all-zero volume
        const TrackRec rec = recs ? recs[b] : TrackRec{{0, P.half_a, 0, 0}, 0, {0, 0, 0}};
        const float* g = guesses + 3 * b;
        const float* rt = st.rot + 2 * st.A * b;
        dpg_track_result r;
        memset(&r, 0, sizeof(r));
        r.pose[0] = (float)((double)((int64_t)st.scans[b].cx + rec.win.dx) * m->res);
        r.pose[1] = (float)((double)((int64_t)st.scans[b].cy + rec.win.dy) * m->res);
        r.pose[2] = (float)((double)g[2] + (double)(rec.win.a - P.half_a) * (double)P.angle_step);
        r.rot[0] = rt[2 * rec.win.a];
        r.rot[1] = rt[2 * rec.win.a + 1];
        r.score = rec.win.score;
        r.score_at_guess = rec.score_at_guess;
        r.n_pts = (int32_t)(st.scans[b].end - st.scans[b].begin);
        r.best_a = rec.win.a; r.best_dx = rec.win.dx; r.best_dy = rec.win.dy;
        r.status = rec.win.score == 0 ? DPG_LOC_NO_OVERLAP : DPG_LOC_OK;
        out[b] = r;
    }
}

extern "C" float dpg_fmap_track_kernel_ms(const dpg_fmap* m) { return m ? m->track_ms : 0.f; }

extern "C" int dpg_fmap_track(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                              const dpg_track_params* p, dpg_track_result* out) {
    const char* who = "dpg_fmap_track";
    if (int rc = track_check(m, clouds, offsets, B, guesses, p, out, who)) return rc;
    if (B == 0) return DPG_OK;
    TrackStage st;
    if (int rc = track_stage(m, clouds, offsets, B, guesses, p, who, st)) return rc;
    if (m->h_recs.reserve((size_t)B)) return fail(DPG_ERR_HIP, "%s: out of pinned memory for %lld scans", who, (long long)B);
    const bool empty = m->cells() == 0;
    if (!empty) {
        hipStream_t s = m->s;
        if (m->d_in.reserve(st.n_in) || m->recs.reserve((size_t)B))
            return fail(DPG_ERR_HIP, "%s: out of device memory for %lld scans", who, (long long)B);
        for (DevEvent& e : m->track_ev)
            if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
        HIP_TRY(hipMemcpyAsync(m->d_in.p, m->h_in.p, st.n_in, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(m->track_ev[0].e, s));
        if (int rc = track_launch(m, st, m->recs.p, who)) return rc;
        HIP_TRY(hipEventRecord(m->track_ev[1].e, s));
        HIP_TRY(hipMemcpyAsync(m->h_recs.p, m->recs.p, sizeof(TrackRec) * (size_t)B, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&m->track_ms, m->track_ev[0].e, m->track_ev[1].e);
    }
    track_results(m, st, guesses, empty ? nullptr : m->h_recs.p, out);
    return DPG_OK;
}
