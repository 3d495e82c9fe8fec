// dpg_csm.hip -- correlative scan matching (Olson 2009) for loop-closure guesses, batched: the kernel
// and its extern "C" entry points (dpg_csm_batch / _table / _scores / _kernel_ms).  The contract --
// smoothing table, cell keys, rotations, score, tie order, refined guess -- is the comment above
// dpg_csm_params in include/dpg_slam_c.h; the host halves (dpg_csm_lut, dpg_csm_rotations,
// dpg_csm_lds_bytes) are plain C in dpg_host.c.  The reference has no such stage.
//
// One workgroup of kT threads per pair.  LDS carve (dynamic, dpg_csm_lds_bytes):
//   [0, tb)            the target's table as bytes, Wp x Hp with Wp = 2H + 1 + 4hx, Hp = 2H + 1 + 4hy:
//                      the table proper (side 2H + 1) inside a zero apron of ax = 2hx columns and
//                      ay = 2hy rows on every side; tb = Wp Hp rounded up to 16
//   [tb, +8192)        kChunk packed cells of the current chunk of points
//   [.., +1280)        the smoothing stencil: 64 pass starts, then up to 256 entries
//   [.., +64)          the chunk's point count, the workgroup's best key, the score at the guess
// Table build: per chunk of target points, the points whose key lies within R of the table are
// compacted into the cell list; then one pass per distinct d2 of the stencil, a barrier between
// passes.  All writers of a pass write the same byte, and a writer stores only over a smaller byte,
// so after the pass every touched cell holds max(before, byte) whichever writer came last: no
// atomics, identical bytes every run, and chunks may come in any order.
// Scoring: per angle the source points' cells are computed once per chunk into LDS (compacted: a
// point whose unshifted key lies more than the window outside the table can reach it under no shift
// and is dropped, exactly); each thread owns one shift (dx, dy), lanes along dx with a window row
// padded to whole lane groups, and walks the list -- the packed cell is a broadcast read, the table
// byte of neighbouring lanes a neighbouring byte.  The apron removes
// the bounds test: a kept point's shifted cell is always inside the padded table (bounds below).
// Every loop is bounded by the validated parameters and the pair's point counts; no workgroup waits
// for another.

#include <math.h>
#include <string.h>

#include "dpg_raster.h"   // cell_key

namespace {

constexpr int kT = 1024;             // threads per workgroup
constexpr int kChunk = 2048;         // points per LDS chunk
constexpr int kStencilStarts = 64;   // pass starts (at most R^2 + 2 = 51 used)
constexpr int kStencilWords = 320;   // starts + entries (at most 15 x 15 = 225 used)
constexpr int kScalBytes = 64;
static_assert(kChunk * 4 + kStencilWords * 4 + kScalBytes == DPG_CSM_LDS_FIXED, "the header's LDS formula");

struct CsmArgs {
    const float2* ds;             // the store's downsampled clouds
    const dpg_csm_pair* pairs;    // [grid]
    const float* rot;             // [grid][2 ha + 1][2]
    const int32_t* stencil;       // [kStencilWords]
    dpg_csm_result* res;          // [grid]
    uint8_t* table_out;           // diagnostic: [grid][2H + 1][2H + 1], the kernel stops after the build
    int32_t* vol_out;             // diagnostic: [grid][2 ha + 1][2 hy + 1][2 hx + 1]
    double res_m;                 // (double)resolution
    int32_t H, hx, hy, ha, R, n_passes;
};

__global__ __launch_bounds__(kT) void csm_kernel(CsmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;
    const dpg_csm_pair P = a.pairs[pair];
    const int H = a.H, hx = a.hx, hy = a.hy, R = a.R;
    const int ax = 2 * hx, ay = 2 * hy;
    const int Wp = 2 * H + 1 + 2 * ax, Hp = 2 * H + 1 + 2 * ay;
    const int tb = (Wp * Hp + 15) / 16 * 16;
    uint8_t* tbl = smem;
    uint32_t* cells = reinterpret_cast<uint32_t*>(smem + tb);
    int32_t* sten = reinterpret_cast<int32_t*>(smem + tb + kChunk * 4);
    unsigned long long* s_best = reinterpret_cast<unsigned long long*>(smem + tb + kChunk * 4 + kStencilWords * 4);
    int32_t* s_cnt = reinterpret_cast<int32_t*>(s_best + 1);
    int32_t* s_at_guess = s_cnt + 1;

    for (int i = tid; i < tb / 4; i += kT) reinterpret_cast<uint32_t*>(tbl)[i] = 0u;
    for (int i = tid; i < kStencilWords; i += kT) sten[i] = a.stencil[i];
    if (tid == 0) {
        *s_best = 0ull;
        *s_at_guess = 0;
    }
    __syncthreads();

    // ---- the table of the target ----
    for (int c0 = 0; c0 < P.n_tgt; c0 += kChunk) {
        if (tid == 0) *s_cnt = 0;   // the last readers of s_cnt passed a pass barrier (n_passes >= 1)
        __syncthreads();
        const int c1 = min(c0 + kChunk, P.n_tgt);
        for (int i = c0 + tid; i < c1; i += kT) {
            const float2 p = a.ds[P.tgt_off + i];
            int kx, ky;
            if (!cell_key(p.x, p.y, a.res_m, kx, ky)) continue;
            if (abs(kx) > H + R || abs(ky) > H + R) continue;   // its stencil cannot reach the table
            // slot < kChunk: at most c1 - c0 <= kChunk points append; both halves in [0, 2H + 2R] < 2^16
            const int slot = atomicAdd(s_cnt, 1);
            cells[slot] = (uint32_t)(kx + H + R) | (uint32_t)(ky + H + R) << 16;
        }
        __syncthreads();
        const int n = *s_cnt;
        for (int pass = 0; pass < a.n_passes; ++pass) {
            const int s0 = sten[pass], ne = sten[pass + 1] - s0;   // pass + 1 <= 50 < kStencilStarts
            const int work = n * ne;                               // <= 2048 * 225
            for (int w = tid; w < work; w += kT) {
                const int pt = w / ne;
                const int32_t e = sten[kStencilStarts + s0 + w % ne];   // s0 + ne <= 225 entries
                const int ox = (int8_t)(e & 0xff), oy = (int8_t)((e >> 8) & 0xff);
                const uint8_t val = (uint8_t)((e >> 16) & 0xff);
                const uint32_t c = cells[pt];
                const int u = (int)(c & 0xffffu) - R + ox, v = (int)(c >> 16) - R + oy;   // key + H
                if ((unsigned)u > (unsigned)(2 * H) || (unsigned)v > (unsigned)(2 * H)) continue;
                // 0 <= v + ay <= 2H + ay < Hp and 0 <= u + ax <= 2H + ax < Wp: inside the table bytes
                const int idx = (v + ay) * Wp + (u + ax);
                if (tbl[idx] < val) tbl[idx] = val;
            }
            __syncthreads();
        }
    }

    if (a.table_out) {
        const int W = 2 * H + 1;
        uint8_t* out = a.table_out + pair * (int64_t)W * W;
        for (int i = tid; i < W * W; i += kT) out[i] = tbl[(i / W + ay) * Wp + (i % W + ax)];
        return;
    }

    // ---- scores ----
    const int Wx = 2 * hx + 1, Wy = 2 * hy + 1, nshift = Wx * Wy, A = 2 * a.ha + 1;
    // lanes per window row: the row's Wx shifts padded to a power of two up to 32, then to whole
    // groups of 32 lanes, so the 32 lanes the LDS serves together read one table row (neighbouring
    // bytes), not the ends of two rows Wp bytes apart on the same banks; the padding lanes idle
    int lpr = 32;
    if (Wx <= 32) {
        lpr = 1;
        while (lpr < Wx) lpr *= 2;
    } else {
        lpr = (Wx + 31) / 32 * 32;
    }
    const int nlanes = lpr * Wy;
    const float* rot = a.rot + pair * (int64_t)A * 2;
    int32_t* vol = a.vol_out ? a.vol_out + pair * (int64_t)A * nshift : nullptr;
    unsigned long long best = 0ull;
    int best_a = 0, best_j = 0;
    for (int ia = 0; ia < A; ++ia) {
        const float c = rot[2 * ia], s = rot[2 * ia + 1];
        for (int j0 = 0; j0 < nlanes; j0 += kT) {
            const int row = (j0 + tid) / lpr, col = (j0 + tid) % lpr;
            const bool active = row < Wy && col < Wx;
            const int j = row * Wx + col;   // the shift's index in the window, < nshift when active
            const int dx = col - hx, dy = row - hy;
            const int off = dy * Wp + dx;
            int32_t score = 0;
            for (int c0 = 0; c0 < P.n_src; c0 += kChunk) {
                __syncthreads();   // the list's last readers are done
                if (tid == 0) *s_cnt = 0;
                __syncthreads();
                const int c1 = min(c0 + kChunk, P.n_src);
                for (int i = c0 + tid; i < c1; i += kT) {
                    const float2 p = a.ds[P.src_off + i];
                    const float qx = ((c * p.x) - (s * p.y)) + P.tx;
                    const float qy = ((s * p.x) + (c * p.y)) + P.ty;
                    int kx, ky;
                    if (!cell_key(qx, qy, a.res_m, kx, ky)) continue;
                    if (abs(kx) > H + hx || abs(ky) > H + hy) continue;   // no shift brings it into the table
                    // px = kx + H + ax in [hx, 2H + 3hx], py = ky + H + ay in [hy, 2H + 3hy]
                    const int slot = atomicAdd(s_cnt, 1);   // < kChunk as above
                    cells[slot] = (uint32_t)((ky + H + ay) * Wp + (kx + H + ax));
                }
                __syncthreads();
                if (active) {
                    // base + off = (py + dy) Wp + (px + dx) with 0 <= px + dx <= 2H + 4hx = Wp - 1 and
                    // 0 <= py + dy <= Hp - 1: inside the table bytes for every |dx| <= hx, |dy| <= hy
                    const int n = *s_cnt;
                    int i = 0;
                    for (; i + 4 <= n; i += 4) {
                        const uint4 b = *reinterpret_cast<const uint4*>(cells + i);
                        score += (int32_t)tbl[(int)b.x + off] + (int32_t)tbl[(int)b.y + off] +
                                 (int32_t)tbl[(int)b.z + off] + (int32_t)tbl[(int)b.w + off];
                    }
                    for (; i < n; ++i) score += (int32_t)tbl[(int)cells[i] + off];
                }
            }
            if (!active) continue;
            if (vol) vol[ia * nshift + j] = score;
            if (ia == a.ha && dx == 0 && dy == 0) *s_at_guess = score;
            // the score, then the tie order as bits where larger is better: |a - ha| (7 bits), dx^2 + dy^2
            // (14), a below the centre (1), dy (8), dx not positive (1); (a, dx, dy) -> key is one to one
            const int da = abs(ia - a.ha), d2 = dx * dx + dy * dy;
            const unsigned long long key = (unsigned long long)score << 31 | (unsigned long long)(127 - da) << 24 |
                                           (unsigned long long)(16383 - d2) << 10 |
                                           (unsigned long long)(ia <= a.ha ? 1 : 0) << 9 |
                                           (unsigned long long)(255 - (dy + hy)) << 1 | (unsigned long long)(dx <= 0 ? 1 : 0);
            if (key > best) {
                best = key;
                best_a = ia;
                best_j = j;
            }
        }
    }
    if (best) atomicMax(s_best, best);
    __syncthreads();
    if (best && best == *s_best) {   // one thread: the keys are distinct
        const int dx = best_j % Wx - hx, dy = best_j / Wx - hy;
        const float c = rot[2 * best_a], s = rot[2 * best_a + 1];
        dpg_csm_result r;
        r.guess[0] = c;
        r.guess[1] = -s;
        r.guess[2] = (float)((double)P.tx + (double)dx * a.res_m);
        r.guess[3] = s;
        r.guess[4] = c;
        r.guess[5] = (float)((double)P.ty + (double)dy * a.res_m);
        r.score = (int32_t)(best >> 31);
        r.score_at_guess = *s_at_guess;
        r.n_src = P.n_src;
        r.best_a = best_a;
        r.best_dx = dx;
        r.best_dy = dy;
        r.status = r.score > 0 ? DPG_CSM_OK : DPG_CSM_NO_OVERLAP;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        a.res[pair] = r;
    }
}

// the smoothing stencil for the kernel: sten[p] = first entry of pass p (sten[n_passes] = the entry
// count), entries from kStencilStarts on as ox | oy << 8 | lut[d2] << 16, one pass per d2 with a
// non-zero byte, largest d2 first; returns n_passes (>= 1: lut[0] = 255)
int build_stencil(const dpg_csm_params& P, std::vector<int32_t>& sten) {
    uint8_t lut[50];
    dpg_csm_lut(&P, lut);
    sten.assign(kStencilWords, 0);
    const int R = P.kernel_radius;
    int n_passes = 0, n = 0;
    for (int d2 = R * R; d2 >= 0; --d2) {
        if (!lut[d2]) continue;
        const int first = n;
        for (int oy = -R; oy <= R; ++oy)
            for (int ox = -R; ox <= R; ++ox)
                if (ox * ox + oy * oy == d2) sten[(size_t)(kStencilStarts + n++)] = (ox & 0xff) | (oy & 0xff) << 8 | (int32_t)lut[d2] << 16;
        if (n > first) sten[(size_t)n_passes++] = first;
    }
    sten[(size_t)n_passes] = n;
    return n_passes;
}

int check_params(dpg_ctx* c, const dpg_csm_params* p, const char* who) {
    if (!c) return fail(DPG_ERR_ARG, "%s: ctx is NULL", who);
    if (is_multi(c)) return fail(DPG_ERR_STATE, "%s runs on a single-device context", who);
    if (!p) return fail(DPG_ERR_ARG, "%s: params is NULL", who);
    if (dpg_csm_lds_bytes(p) < 0)
        return fail(DPG_ERR_ARG, "%s: an invalid field, or a table and window above the kernel's %d bytes of LDS", who,
                    DPG_CSM_LDS_BUDGET);
    if (c->n_nodes <= 0) return fail(DPG_ERR_STATE, "no scans uploaded");
    return DPG_OK;
}

int fill_pair(dpg_ctx* c, int32_t t, int32_t s, const float g[6], dpg_csm_pair& q) {
    if (t < 0 || s < 0 || t >= c->n_nodes || s >= c->n_nodes) return DPG_ERR_ARG;
    memset(&q, 0, sizeof(q));
    q.tgt_off = (int32_t)c->ds_off[(size_t)t];
    q.n_tgt = (int32_t)(c->ds_off[(size_t)t + 1] - c->ds_off[(size_t)t]);
    q.src_off = (int32_t)c->ds_off[(size_t)s];
    q.n_src = (int32_t)(c->ds_off[(size_t)s + 1] - c->ds_off[(size_t)s]);
    q.tx = g[2];
    q.ty = g[5];
    return q.n_src > 16384 || q.n_tgt > 16384 ? DPG_ERR_SIZE : DPG_OK;
}

// launch over `pairs` (rot: their rotation tables) and copy back what is asked for; blocks
int run(dpg_ctx* c, const dpg_csm_params& P, const std::vector<dpg_csm_pair>& pairs, const std::vector<float>& rot,
        dpg_csm_result* res_host, uint8_t* table_host, int32_t* vol_host) {
    const size_t E = pairs.size();
    if (E == 0) return DPG_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> sten;
    const int n_passes = build_stencil(P, sten);
    const size_t W = 2 * (size_t)P.half_cells + 1;
    const size_t A = 2 * (size_t)P.half_a + 1, nshift = (2 * (size_t)P.half_x + 1) * (2 * (size_t)P.half_y + 1);
    const size_t diag = table_host ? (E * W * W + 3) / 4 : vol_host ? E * A * nshift : 0;
    if (c->csm_pairs.reserve(E) || c->csm_rot.reserve(std::max<size_t>(rot.size(), 1)) ||
        c->csm_stencil.reserve(kStencilWords) || c->csm_res.reserve(E) || c->csm_diag.reserve(diag))
        return fail(DPG_ERR_HIP, "out of device memory for %zu scan-matching pairs", E);
    if (c->csm_ev[0].ensure(hipEventDefault) || c->csm_ev[1].ensure(hipEventDefault))
        return fail(DPG_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipMemcpyAsync(c->csm_pairs.p, pairs.data(), sizeof(dpg_csm_pair) * E, hipMemcpyHostToDevice, c->stream));
    if (!rot.empty())
        HIP_TRY(hipMemcpyAsync(c->csm_rot.p, rot.data(), sizeof(float) * rot.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->csm_stencil.p, sten.data(), sizeof(int32_t) * kStencilWords, hipMemcpyHostToDevice, c->stream));
    CsmArgs a;
    a.ds = reinterpret_cast<const float2*>(c->ds.p);
    a.pairs = c->csm_pairs.p;
    a.rot = c->csm_rot.p;
    a.stencil = c->csm_stencil.p;
    a.res = c->csm_res.p;
    a.table_out = table_host ? reinterpret_cast<uint8_t*>(c->csm_diag.p) : nullptr;
    a.vol_out = vol_host ? c->csm_diag.p : nullptr;
    a.res_m = (double)P.resolution;
    a.H = P.half_cells;
    a.hx = P.half_x;
    a.hy = P.half_y;
    a.ha = P.half_a;
    a.R = P.kernel_radius;
    a.n_passes = n_passes;
    const size_t lds = (size_t)dpg_csm_lds_bytes(&P);
    // more than 64 KiB of dynamic LDS: raise the kernel's limit where the runtime keeps one (its answer
    // does not matter: the launch below reports what the device refuses)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(csm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipGetLastError();
    c->csm_timed = false;
    HIP_TRY(hipEventRecord(c->csm_ev[0].e, c->stream));
    hipLaunchKernelGGL(csm_kernel, dim3((unsigned)E), dim3(kT), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->csm_ev[1].e, c->stream));
    c->csm_timed = true;
    if (res_host)
        HIP_TRY(hipMemcpyAsync(res_host, c->csm_res.p, sizeof(dpg_csm_result) * E, hipMemcpyDeviceToHost, c->stream));
    if (table_host) HIP_TRY(hipMemcpyAsync(table_host, c->csm_diag.p, E * W * W, hipMemcpyDeviceToHost, c->stream));
    if (vol_host)
        HIP_TRY(hipMemcpyAsync(vol_host, c->csm_diag.p, sizeof(int32_t) * E * A * nshift, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DPG_OK;
}

}  // namespace

extern "C" {

int dpg_csm_batch(dpg_ctx* c, const int32_t* edges, int64_t ne, const float* poses, const float* guesses,
                  const dpg_csm_params* p, dpg_csm_result* out, int64_t cap) {
    int rc = check_params(c, p, "dpg_csm_batch");
    if (rc) return rc;
    if (ne < 0 || (ne > 0 && (!edges || !out))) return fail(DPG_ERR_ARG, "dpg_csm_batch: bad arguments");
    if ((poses != nullptr) == (guesses != nullptr))
        return fail(DPG_ERR_ARG, "dpg_csm_batch: exactly one of poses and guesses must be given");
    if (cap < ne) return fail(DPG_ERR_SIZE, "dpg_csm_batch: results_out holds %lld records, the batch has %lld", (long long)cap, (long long)ne);
    const size_t A = 2 * (size_t)p->half_a + 1;
    std::vector<dpg_csm_pair> pairs((size_t)ne);
    std::vector<float> rot((size_t)ne * A * 2);
    for (int64_t e = 0; e < ne; ++e) {
        const int32_t t = edges[2 * e], s = edges[2 * e + 1];
        if (t < 0 || s < 0 || t >= c->n_nodes || s >= c->n_nodes)
            return fail(DPG_ERR_ARG, "edge %lld references a missing node", (long long)e);
        float g[6];
        if (poses) dpg_icp_guess(poses + 3 * s, poses + 3 * t, g);
        else memcpy(g, guesses + 6 * e, sizeof(g));
        if ((rc = fill_pair(c, t, s, g, pairs[(size_t)e]))) return fail(rc, "edge %lld: a cloud above 16384 points", (long long)e);
        dpg_csm_rotations(g, p, rot.data() + (size_t)e * A * 2);
    }
    std::vector<dpg_csm_result> res((size_t)ne);   // the caller's array is written only on success
    if ((rc = run(c, *p, pairs, rot, res.data(), nullptr, nullptr))) return rc;
    if (ne > 0) memcpy(out, res.data(), sizeof(dpg_csm_result) * (size_t)ne);
    return DPG_OK;
}

int dpg_csm_table(dpg_ctx* c, int32_t node, const dpg_csm_params* p, uint8_t* out, int64_t cap) {
    int rc = check_params(c, p, "dpg_csm_table");
    if (rc) return rc;
    if (!out) return fail(DPG_ERR_ARG, "dpg_csm_table: out is NULL");
    const int64_t W = 2 * (int64_t)p->half_cells + 1;
    if (cap < W * W) return fail(DPG_ERR_SIZE, "dpg_csm_table: out holds %lld bytes, the table has %lld", (long long)cap, (long long)(W * W));
    const float g[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    std::vector<dpg_csm_pair> pairs(1);
    if ((rc = fill_pair(c, node, node, g, pairs[0]))) return fail(rc, "dpg_csm_table: node %d is missing or too large", node);
    pairs[0].n_src = 0;
    return run(c, *p, pairs, std::vector<float>(), nullptr, out, nullptr);
}

int dpg_csm_scores(dpg_ctx* c, int32_t target, int32_t source, const float guess[6], const dpg_csm_params* p,
                   int32_t* out, int64_t cap) {
    int rc = check_params(c, p, "dpg_csm_scores");
    if (rc) return rc;
    if (!out || !guess) return fail(DPG_ERR_ARG, "dpg_csm_scores: bad arguments");
    const int64_t A = 2 * (int64_t)p->half_a + 1, n = A * (2 * (int64_t)p->half_x + 1) * (2 * (int64_t)p->half_y + 1);
    if (cap < n) return fail(DPG_ERR_SIZE, "dpg_csm_scores: out holds %lld scores, the volume has %lld", (long long)cap, (long long)n);
    std::vector<dpg_csm_pair> pairs(1);
    if ((rc = fill_pair(c, target, source, guess, pairs[0])))
        return fail(rc, "dpg_csm_scores: a node is missing or above 16384 points");
    std::vector<float> rot((size_t)A * 2);
    dpg_csm_rotations(guess, p, rot.data());
    return run(c, *p, pairs, rot, nullptr, nullptr, out);
}

float dpg_csm_kernel_ms(dpg_ctx* c) {
    float ms = -1.f;
    if (!c || !c->csm_timed || hipEventSynchronize(c->csm_ev[1].e) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->csm_ev[0].e, c->csm_ev[1].e) != hipSuccess) return -1.f;
    return ms;
}

}  // extern "C"
