// dpg_refine.hip -- dpg_fmap_refine / dpg_fmap_track_refine: sub-cell pose refinement of a batch of
// scans on a frozen map's interpolated field, a few damped Gauss-Newton steps per scan, in one
// enqueue.  The contract is the comment above dpg_refine_params in include/dpg_slam_c.h; every fp64
// expression stands as written there (-ffp-contract=off), and the host's part (start checks, record,
// covariance) is plain C in dpg_host.c.  The reference has no such stage.
//
//   refine_kernel   a workgroup of 256 threads = one scan, resident for all its evaluations.  A scan
//                   of <= 2048 points sits in LDS as float2 (16 KiB); a longer one is read again from
//                   global memory at every evaluation.  A lane gathers the four bytes of its point
//                   through L2 and keeps the eleven fp64 partial sums and the count in registers;
//                   a wave folds them by shuffles in the contract's order, the four wave partials meet
//                   in LDS, and lane 0 adds them, keeps the best iterate, takes the step (a dependent
//                   chain of nine fp64 divisions) and publishes the next state in LDS: two barriers
//                   per evaluation.  kFromTrack: the start is derived from the scan's track record,
//                   which the launch before it on the same stream has written.
// Every loop is bounded by the validated parameters and the offsets, every field index is tested
// against the box at its access, no workgroup waits for another and there is no atomic.

#include <math.h>
#include <string.h>

#include "dpg_loc_dev.h"

namespace {

constexpr int kRefS = 11;                      // the sums of an evaluation
constexpr int kRefCols = DPG_REFINE_TRACE_COLS;
constexpr double kRefLim = 536870912.0;        // 2^29
static_assert(kRefCols == 4 + kRefS + 1, "a trace row: the state, the sums, n_used");

struct RefineDims {
    int32_t w, h, x0, y0;      // F [h][w]
    int32_t max_iters, A;      // A: the tracker's angles (kFromTrack)
    double res, ires;
    double lambda, max_cells, max_angle, tol_cells, tol_angle;
};

// one scan as the kernel reads it without a track record: its points [begin, end) and its start
struct RefineScan { int64_t begin, end; float x, y, c, s; };

// what the device leaves of a scan: dpg_refine_record's arguments
struct RefineRec {
    int32_t status, n_evals, best_eval, n_used;
    double state[4];
    double S[kRefS];
    double cost_start;
};

__device__ __forceinline__ double field_at(const uint8_t* F, int32_t w, int32_t h, int x, int y) {
    return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? (double)F[(int64_t)y * w + x] : 0.0;
}

__device__ __forceinline__ double clamp_pm(double z, double m) { return z > m ? m : (z < -m ? -m : z); }

// grid B
template <bool kFromTrack>
__global__ __launch_bounds__(kLocT) void refine_kernel(RefineDims g, const RefineScan* scans, const TrackScan* tscans, const TrackRec* trk,
                                                       const float* rot, const float2* cloud, const uint8_t* F, RefineRec* recs,
                                                       double* trace) {
    __shared__ float2 s_pts[kLocChunk];
    __shared__ double s_part[kLocT / 64][kRefS];
    __shared__ int32_t s_cnt[kLocT / 64];
    __shared__ double s_state[4];
    __shared__ int32_t s_stop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;                                    // b < B
    int64_t begin, end;
    if (kFromTrack) {
        begin = tscans[b].begin;
        end = tscans[b].end;
    } else {
        begin = scans[b].begin;
        end = scans[b].end;
    }
    const int64_t n = end - begin;                                   // 0 .. 2^23
    const bool in_lds = n <= kLocChunk;
    if (in_lds)
        for (int i = tid; i < (int)n; i += kLocT) s_pts[i] = cloud[begin + i];
    if (tid == 0) {
        float x, y, c, s;
        if (kFromTrack) {
            const TrackRec t = trk[b];                               // a < A
            x = (float)((double)((int64_t)tscans[b].cx + t.win.dx) * g.res);
            y = (float)((double)((int64_t)tscans[b].cy + t.win.dy) * g.res);
            c = rot[(b * g.A + t.win.a) * 2];
            s = rot[(b * g.A + t.win.a) * 2 + 1];
        } else {
            x = scans[b].x; y = scans[b].y; c = scans[b].c; s = scans[b].s;
        }
        s_state[0] = ((double)x * g.ires) - (double)g.x0;
        s_state[1] = ((double)y * g.ires) - (double)g.y0;
        s_state[2] = (double)c;
        s_state[3] = (double)s;
        s_stop = 0;
    }
    __syncthreads();
    RefineRec* out = recs + b;
    double* tr = trace ? trace + b * (int64_t)(g.max_iters + 1) * kRefCols : nullptr;
    double best_cost = 0.0;                                          // lane 0's
    for (int k = 0; k <= g.max_iters; ++k) {                         // uniform over the workgroup
        const double tu = s_state[0], tv = s_state[1], c = s_state[2], s = s_state[3];
        double S[kRefS];
#pragma unroll
        for (int j = 0; j < kRefS; ++j) S[j] = 0.0;
        int32_t cnt = 0;
        for (int64_t i = tid; i < n; i += kLocT) {
            const float2 p = in_lds ? s_pts[i] : cloud[begin + i];
            if (!(fabsf(p.x) <= 3.402823466e+38f) || !(fabsf(p.y) <= 3.402823466e+38f)) continue;   // not finite
            const double px = (double)p.x * g.ires, py = (double)p.y * g.ires;
            const double rx = (c * px) - (s * py), ry = (s * px) + (c * py);
            const double u = rx + tu, v = ry + tv;
            if (!(fabs(u) < kRefLim) || !(fabs(v) < kRefLim)) continue;
            const double flu = floor(u), flv = floor(v);
            const int iu = (int)flu, iv = (int)flv;                  // |.| <= 2^29
            const double fu = u - flu, fv = v - flv, au = 1.0 - fu, av = 1.0 - fv;
            const double F00 = field_at(F, g.w, g.h, iu, iv), F10 = field_at(F, g.w, g.h, iu + 1, iv);
            const double F01 = field_at(F, g.w, g.h, iu, iv + 1), F11 = field_at(F, g.w, g.h, iu + 1, iv + 1);
            const double M = (av * ((au * F00) + (fu * F10))) + (fv * ((au * F01) + (fu * F11)));
            const double gu = (av * (F10 - F00)) + (fv * (F11 - F01));
            const double gv = (au * (F01 - F00)) + (fu * (F11 - F10));
            const double r = 255.0 - M, jt = (gv * rx) - (gu * ry);
            S[0] += gu * gu; S[1] += gu * gv; S[2] += gu * jt;
            S[3] += gv * gv; S[4] += gv * jt; S[5] += jt * jt;
            S[6] += gu * r;  S[7] += gv * r;  S[8] += jt * r;
            S[9] += r * r;   S[10] += r;
            ++cnt;
        }
        // the wave's fold: p[l] += p[l + stride] for l < stride (the lanes above hold values nobody reads)
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) {
#pragma unroll
            for (int j = 0; j < kRefS; ++j) S[j] += __shfl_down(S[j], st, 64);
            cnt += __shfl_down(cnt, st, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < kRefS; ++j) s_part[wave][j] = S[j];
            s_cnt[wave] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            double T[kRefS];
#pragma unroll
            for (int j = 0; j < kRefS; ++j) T[j] = (s_part[0][j] + s_part[1][j]) + (s_part[2][j] + s_part[3][j]);
            const int32_t n_used = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            if (tr) {
                double* row = tr + (int64_t)k * kRefCols;
                row[0] = tu; row[1] = tv; row[2] = c; row[3] = s;
#pragma unroll
                for (int j = 0; j < kRefS; ++j) row[4 + j] = T[j];
                row[4 + kRefS] = (double)n_used;
            }
            if (k == 0 || T[9] < best_cost) {
                best_cost = T[9];
                out->best_eval = k;
                out->n_used = n_used;
                out->state[0] = tu; out->state[1] = tv; out->state[2] = c; out->state[3] = s;
#pragma unroll
                for (int j = 0; j < kRefS; ++j) out->S[j] = T[j];
                if (k == 0) out->cost_start = T[9];
            }
            int status = -1;
            if (k == 0 && n_used == 0) status = DPG_REFINE_NO_POINTS;
            else if (k == g.max_iters) status = DPG_REFINE_MAX_ITERS;
            else {
                const double eps = 1e-12;
                const double H00 = T[0], H01 = T[1], H02 = T[2], H11 = T[3], H12 = T[4], H22 = T[5];
                const double D1 = H11 + (g.lambda * H11), D2 = H22 + (g.lambda * H22);
                const double d0 = H00 + (g.lambda * H00);
                bool ok = d0 > 0.0;
                double z0 = 0.0, z1 = 0.0, z2 = 0.0;
                if (ok) {
                    const double l10 = H01 / d0, l20 = H02 / d0;
                    const double d1 = D1 - (l10 * H01);
                    ok = d1 > eps * D1;
                    if (ok) {
                        const double e12 = H12 - (l20 * H01), l21 = e12 / d1;
                        const double d2 = (D2 - (l20 * H02)) - (l21 * e12);
                        ok = d2 > eps * D2;
                        if (ok) {
                            const double y0 = T[6], y1 = T[7] - (l10 * y0), y2 = (T[8] - (l20 * y0)) - (l21 * y1);
                            z2 = y2 / d2;
                            z1 = (y1 / d1) - (l21 * z2);
                            z0 = ((y0 / d0) - (l10 * z1)) - (l20 * z2);
                            ok = fabs(z0) < INFINITY && fabs(z1) < INFINITY && fabs(z2) < INFINITY;   // finite
                        }
                    }
                }
                if (!ok) status = DPG_REFINE_DEGENERATE;
                else {
                    const double du = clamp_pm(z0, g.max_cells), dv = clamp_pm(z1, g.max_cells), dt = clamp_pm(z2, g.max_angle);
                    if (fabs(du) < g.tol_cells && fabs(dv) < g.tol_cells && fabs(dt) < g.tol_angle) status = DPG_REFINE_CONVERGED;
                    else {
                        const double a = dt * 0.5, q = a * a, den = 1.0 + q;
                        const double cd = (1.0 - q) / den, sd = (a + a) / den;
                        s_state[0] = tu + du;
                        s_state[1] = tv + dv;
                        s_state[2] = (c * cd) - (s * sd);
                        s_state[3] = (s * cd) + (c * sd);
                    }
                }
            }
            if (status >= 0) {
                out->status = status;
                out->n_evals = k + 1;
                s_stop = 1;
                if (tr)                                              // rows past n_evals are zero
                    for (int64_t i = (int64_t)(k + 1) * kRefCols; i < (int64_t)(g.max_iters + 1) * kRefCols; ++i) tr[i] = 0.0;
            }
        }
        __syncthreads();
        if (s_stop) break;                                           // uniform: written before the barrier
    }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

RefineDims refine_dims(const dpg_fmap* m, const dpg_refine_params& P, int64_t A) {
    RefineDims g;
    memset(&g, 0, sizeof(g));
    g.w = m->box[2]; g.h = m->box[3]; g.x0 = m->box[0]; g.y0 = m->box[1];
    g.max_iters = P.max_iters;
    g.A = (int32_t)A;
    g.res = m->res;
    g.ires = 1.0 / m->res;
    g.lambda = P.lambda; g.max_cells = P.max_step_cells; g.max_angle = P.max_step_angle;
    g.tol_cells = P.tol_cells; g.tol_angle = P.tol_angle;
    return g;
}

size_t trace_doubles(int64_t B, const dpg_refine_params& P) { return (size_t)B * (size_t)(P.max_iters + 1) * kRefCols; }

// the device's records in pinned memory to the caller's
void refine_results(const dpg_fmap* m, int64_t B, const RefineRec* recs, dpg_refine_result* out) {
    for (int64_t b = 0; b < B; ++b) {
        const RefineRec& r = recs[b];
        dpg_refine_record(r.status, r.n_evals, r.best_eval, r.n_used, r.state, r.S, r.cost_start, m->box, m->res, out + b);
    }
}

int refine_run(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* starts, const dpg_refine_params* p,
               dpg_refine_result* out, bool want_trace, double* trace, int64_t cap, const char* who) {
    if (!m || !p || !offsets || B < 0 || (B > 0 && (!starts || !out))) return fail(DPG_ERR_ARG, "%s: a NULL argument or B < 0", who);
    if (is_multi(m->ctx)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    if (dpg_refine_params_check(p)) return fail(DPG_ERR_ARG, "%s: a parameter out of range", who);
    if (B > 65535) return fail(DPG_ERR_SIZE, "%s: %lld scans, at most 65535 in a call", who, (long long)B);
    if (offsets[0] < 0) return fail(DPG_ERR_ARG, "%s: offsets[0] is negative", who);
    for (int64_t b = 0; b < B; ++b)
        if (offsets[b + 1] < offsets[b]) return fail(DPG_ERR_ARG, "%s: offsets are not monotone at scan %lld", who, (long long)b);
    for (int64_t b = 0; b < B; ++b)
        if (offsets[b + 1] - offsets[b] > (int64_t)1 << 23) return fail(DPG_ERR_SIZE, "%s: scan %lld has more than 2^23 points", who, (long long)b);
    const int64_t total = offsets[B] - offsets[0];
    if (total > (int64_t)1 << 26) return fail(DPG_ERR_SIZE, "%s: %lld points in all, at most 2^26", who, (long long)total);
    if (total > 0 && !clouds) return fail(DPG_ERR_ARG, "%s: clouds_xy is NULL", who);
    const dpg_refine_params P = *p;
    const size_t n_trace = want_trace ? trace_doubles(B, P) : 0;
    if (want_trace && (cap < 0 || (size_t)cap < n_trace || (n_trace > 0 && !trace)))
        return fail(DPG_ERR_SIZE, "%s: the trace holds %lld doubles, %lld are needed", who, (long long)cap, (long long)n_trace);
    const double ires = 1.0 / m->res;
    for (int64_t b = 0; b < B; ++b)
        if (dpg_refine_start_check(starts + 5 * b, ires))
            return fail(DPG_ERR_ARG, "%s: the start of scan %lld is not finite, beyond 2^29 cells or its (c, s) is no rotation", who, (long long)b);
    if (B == 0) return DPG_OK;
    // the upload, one block: scans [B] | the points from offsets[0] on; the results, one block: records [B] | trace
    const size_t o_pts = align16(sizeof(RefineScan) * (size_t)B), n_in = align16(o_pts + sizeof(float) * 2 * (size_t)total);
    const size_t o_trace = align16(sizeof(RefineRec) * (size_t)B), n_out = o_trace + sizeof(double) * n_trace;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = m->s;
    HIP_TRY(hipStreamSynchronize(s));   // the pinned blocks of the previous call are free
    if (m->h_in.reserve(n_in) || m->h_rout.reserve(n_out)) return fail(DPG_ERR_HIP, "%s: out of pinned memory for %lld scans", who, (long long)B);
    if (m->d_in.reserve(n_in) || m->r_out.reserve(n_out)) return fail(DPG_ERR_HIP, "%s: out of device memory for %lld scans", who, (long long)B);
    for (DevEvent& e : m->refine_ev)
        if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
    RefineScan* scans = reinterpret_cast<RefineScan*>(m->h_in.p);
    for (int64_t b = 0; b < B; ++b) {
        const float* st = starts + 5 * b;
        scans[b] = RefineScan{offsets[b] - offsets[0], offsets[b + 1] - offsets[0], st[0], st[1], st[3], st[4]};
    }
    if (total > 0) memcpy(m->h_in.p + o_pts, clouds + 2 * offsets[0], sizeof(float) * 2 * (size_t)total);
    HIP_TRY(hipMemcpyAsync(m->d_in.p, m->h_in.p, n_in, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(m->refine_ev[0].e, s));
    refine_kernel<false><<<(unsigned)B, kLocT, 0, s>>>(refine_dims(m, P, 0), reinterpret_cast<const RefineScan*>(m->d_in.p), nullptr, nullptr, nullptr,
                                                      reinterpret_cast<const float2*>(m->d_in.p + o_pts), m->field.p,
                                                      reinterpret_cast<RefineRec*>(m->r_out.p),
                                                      n_trace ? reinterpret_cast<double*>(m->r_out.p + o_trace) : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->refine_ev[1].e, s));
    HIP_TRY(hipMemcpyAsync(m->h_rout.p, m->r_out.p, n_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&m->refine_ms, m->refine_ev[0].e, m->refine_ev[1].e);
    refine_results(m, B, reinterpret_cast<const RefineRec*>(m->h_rout.p), out);
    if (n_trace) memcpy(trace, m->h_rout.p + o_trace, sizeof(double) * n_trace);
    return DPG_OK;
}

}  // namespace

extern "C" float dpg_fmap_refine_kernel_ms(const dpg_fmap* m) { return m ? m->refine_ms : 0.f; }

extern "C" int dpg_fmap_refine(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* starts,
                               const dpg_refine_params* p, dpg_refine_result* out) {
    return refine_run(m, clouds, offsets, B, starts, p, out, false, nullptr, 0, "dpg_fmap_refine");
}

extern "C" int dpg_fmap_refine_trace(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* starts,
                                     const dpg_refine_params* p, dpg_refine_result* out, double* trace, int64_t cap) {
    return refine_run(m, clouds, offsets, B, starts, p, out, true, trace, cap, "dpg_fmap_refine_trace");
}

extern "C" int dpg_fmap_track_refine(dpg_fmap* m, const float* clouds, const int64_t* offsets, int64_t B, const float* guesses,
                                     const dpg_track_params* tp, const dpg_refine_params* rp, dpg_track_result* track_out,
                                     dpg_refine_result* refine_out) {
    const char* who = "dpg_fmap_track_refine";
    if (!rp || (B > 0 && !refine_out)) return fail(DPG_ERR_ARG, "%s: a NULL argument or B < 0", who);
    if (int rc = track_check(m, clouds, offsets, B, guesses, tp, track_out, who)) return rc;
    if (dpg_refine_params_check(rp)) return fail(DPG_ERR_ARG, "%s: a parameter out of range", who);
    if (B == 0) return DPG_OK;
    TrackStage st;
    if (int rc = track_stage(m, clouds, offsets, B, guesses, tp, who, st)) return rc;
    // every start the window can yield passes dpg_fmap_refine's check: x = (float)((double)(cx + dx) res) is
    // monotone in dx, so the window's two ends decide (c, s are a float cosine and sine)
    const double ires = 1.0 / m->res;
    for (int64_t b = 0; b < B; ++b)
        for (int sg = -1; sg <= 1; sg += 2) {
            const float ends[5] = {(float)((double)((int64_t)st.scans[b].cx + sg * st.P.half_x) * m->res),
                                   (float)((double)((int64_t)st.scans[b].cy + sg * st.P.half_y) * m->res), 0.f, 1.f, 0.f};
            if (dpg_refine_start_check(ends, ires))
                return fail(DPG_ERR_ARG, "%s: the window of scan %lld reaches beyond 2^29 cells", who, (long long)b);
        }
    if (m->cells() == 0) {
        // an empty map: the tracker launches nothing and its records are known here, so the starts are too
        track_results(m, st, guesses, nullptr, track_out);
        std::vector<float> sv((size_t)B * 5);
        for (int64_t b = 0; b < B; ++b) memcpy(&sv[5 * (size_t)b], &track_out[b], sizeof(float) * 5);
        return refine_run(m, clouds, offsets, B, sv.data(), rp, refine_out, false, nullptr, 0, who);
    }
    const dpg_refine_params P = *rp;
    const size_t o_ref = align16(sizeof(TrackRec) * (size_t)B), n_out = o_ref + sizeof(RefineRec) * (size_t)B;
    hipStream_t s = m->s;
    if (m->h_rout.reserve(n_out)) return fail(DPG_ERR_HIP, "%s: out of pinned memory for %lld scans", who, (long long)B);
    if (m->d_in.reserve(st.n_in) || m->r_out.reserve(n_out)) return fail(DPG_ERR_HIP, "%s: out of device memory for %lld scans", who, (long long)B);
    for (DevEvent& e : m->track_ev)
        if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
    for (DevEvent& e : m->refine_ev)
        if (e.ensure(hipEventDefault)) return fail(DPG_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipMemcpyAsync(m->d_in.p, m->h_in.p, st.n_in, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(m->track_ev[0].e, s));
    TrackRec* d_trk = reinterpret_cast<TrackRec*>(m->r_out.p);
    if (int rc = track_launch(m, st, d_trk, who)) return rc;
    HIP_TRY(hipEventRecord(m->track_ev[1].e, s));
    HIP_TRY(hipEventRecord(m->refine_ev[0].e, s));
    refine_kernel<true><<<(unsigned)B, kLocT, 0, s>>>(refine_dims(m, P, st.A), nullptr, reinterpret_cast<const TrackScan*>(m->d_in.p + st.o_scan), d_trk,
                                                     reinterpret_cast<const float*>(m->d_in.p + st.o_rot),
                                                     reinterpret_cast<const float2*>(m->d_in.p + st.o_pts), m->field.p,
                                                     reinterpret_cast<RefineRec*>(m->r_out.p + o_ref), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->refine_ev[1].e, s));
    HIP_TRY(hipMemcpyAsync(m->h_rout.p, m->r_out.p, n_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&m->track_ms, m->track_ev[0].e, m->track_ev[1].e);
    (void)hipEventElapsedTime(&m->refine_ms, m->refine_ev[0].e, m->refine_ev[1].e);
    track_results(m, st, guesses, reinterpret_cast<const TrackRec*>(m->h_rout.p), track_out);
    refine_results(m, B, reinterpret_cast<const RefineRec*>(m->h_rout.p + o_ref), refine_out);
    return DPG_OK;
}
