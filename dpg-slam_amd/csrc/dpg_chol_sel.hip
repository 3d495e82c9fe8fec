// dpg_chol_sel.hip -- covariances from the factor the GPU Cholesky holds, kernels and host sides:
// the selected inverse and the joint marginals.
#include "dpg_chol_dev.h"

using namespace dpg_chol;

namespace {
// ---- selected inverse: the blocks of Sigma = H^-1 inside L's pattern (marginal covariances) ----
// Takahashi's recurrence in multifrontal form, one root-to-leaves pass over the supernodal tree.
// Front s has pivot columns C (k3 scalars) and rows R (r3); with Y = L21 L11^-1 and Z = L11^-1
//   G        = Sigma_parent(relmap(R), relmap(R))        (R lies inside the parent's index set)
//   Sigma_RC = -G Y
//   Sigma_CC = Z^T Z - Y^T Sigma_RC
// and the front's whole (k3 + r3)^2 block [[Sigma_CC, Sigma_RC^T], [Sigma_RC, G]] goes to the Sigma
// buffer (the fronts' layout, full symmetric storage), so a child gathers from its parent alone.
// One launch per elimination-tree level from the roots' down, one workgroup per front: a front's
// parent lies on a higher level, so stream order is the only synchronisation.  No atomics; every
// element is one thread's sum in a fixed order (four accumulators: a dependent fp64 chain costs
// ~32 cycles a step on one wave), so two runs on one factor are bitwise equal.
//   rows:  [Z; Y] = [I; L21] L11^-1, one row per thread by substitution from the right;
//   G Y:   one element per thread, G's column contiguous across the threads;
//   Sigma_CC: lower triangle, one element per thread, mirrored by the same thread.
// A front whose L11, [Z; Y] and Sigma block fit kSelLds doubles (60 KiB, 63 KiB with the table of
// diagonal reciprocals: two workgroups per CU of 160 KiB; 15 block rows always fit, up to 28 with few
// pivot columns) works in LDS (leading dimensions padded to odd) and stores its block once; a larger one (up to
// 381 rows) works in HBM: Sigma in place, [Z; Y] in the work buffer.
constexpr int kSelLds = 7680;
__host__ __device__ inline int sel_pad(int m3) { return m3 | 1; }
__host__ __device__ inline int sel_lds_doubles(int m3, int k3) { return k3 * k3 + sel_pad(m3) * (k3 + m3); }

__global__ __launch_bounds__(kT) void chol_selinv_level(const int32_t* __restrict__ list, const SnDev* __restrict__ sns,
                                                        const int32_t* __restrict__ relmap,
                                                        const int64_t* __restrict__ woff,
                                                        const double* __restrict__ fronts, double* sel, double* work) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double s_rd[384];   // 1 / L(j, j) (k3 <= 381)
    const int tid = threadIdx.x;
    const int32_t s = list[blockIdx.x];
    const SnDev S = sns[s];
    const int k3 = 3 * S.k, r3 = 3 * S.r, m3 = k3 + r3;
    const bool lds = sel_lds_doubles(m3, k3) <= kSelLds;
    const double* F = fronts + S.front_off;
    double* Sg = sel + S.front_off;
    // L11 (leading dimension ll), X = [Z; Y] (m3 x k3, lx), the Sigma block (m3 x m3, lw)
    const double* L11 = F;
    double* X = work + woff[s];
    double* W = Sg;
    int ll = m3, lx = m3, lw = m3;
    if (lds) {
        double* l11 = sm;
        ll = k3;
        lx = lw = sel_pad(m3);
        X = sm + k3 * k3;
        W = X + lx * k3;
        for (int e = tid; e < k3 * k3; e += kT) {
            const int i = e % k3, j = e / k3;
            l11[e] = i >= j ? F[(int64_t)j * m3 + i] : 0.0;
        }
        L11 = l11;
    }
    for (int j = tid; j < k3; j += kT) s_rd[j] = 1.0 / F[(int64_t)j * m3 + j];
    // G from the parent's finished block
    if (r3 > 0) {
        const SnDev Pn = sns[S.parent];
        const int mp3 = 3 * (Pn.k + Pn.r);
        const double* P = sel + Pn.front_off;
        const int32_t* rm = relmap + S.rows_off;
        for (int e = tid; e < r3 * r3; e += kT) {
            const int a = e % r3, b = e / r3;
            const int pa = 3 * rm[a / 3] + a % 3, pb = 3 * rm[b / 3] + b % 3;
            W[(int64_t)(k3 + b) * lw + k3 + a] = P[(int64_t)pb * mp3 + pa];
        }
    }
    __syncthreads();
    // rows of [Z; Y]: x L11 = (e_i | L21(i, :)), columns from the right
    for (int i = tid; i < m3; i += kT) {
        const int jt = i < k3 ? i : k3 - 1;
        for (int j = k3 - 1; j > jt; --j) X[(int64_t)j * lx + i] = 0.0;
        for (int j = jt; j >= 0; --j) {
            const double b = i < k3 ? (j == i ? 1.0 : 0.0) : F[(int64_t)j * m3 + i];
            const double* lc = L11 + (int64_t)j * ll;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int c = j + 1;
            for (; c + 3 <= jt; c += 4) {
                a0 = fma(X[(int64_t)c * lx + i], lc[c], a0);
                a1 = fma(X[(int64_t)(c + 1) * lx + i], lc[c + 1], a1);
                a2 = fma(X[(int64_t)(c + 2) * lx + i], lc[c + 2], a2);
                a3 = fma(X[(int64_t)(c + 3) * lx + i], lc[c + 3], a3);
            }
            for (; c <= jt; ++c) a0 = fma(X[(int64_t)c * lx + i], lc[c], a0);
            X[(int64_t)j * lx + i] = (b - ((a0 + a1) + (a2 + a3))) * s_rd[j];
        }
    }
    __syncthreads();
    // Sigma_RC = -G Y, and its transpose
    for (int e = tid; e < r3 * k3; e += kT) {
        const int i = e % r3, c = e / r3;
        const double* gi = W + (int64_t)k3 * lw + k3 + i;      // G(i, j) at gi[j * lw]
        const double* yc = X + (int64_t)c * lx + k3;            // Y(j, c) at yc[j]
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int j = 0;
        for (; j + 3 < r3; j += 4) {
            a0 = fma(gi[(int64_t)j * lw], yc[j], a0);
            a1 = fma(gi[(int64_t)(j + 1) * lw], yc[j + 1], a1);
            a2 = fma(gi[(int64_t)(j + 2) * lw], yc[j + 2], a2);
            a3 = fma(gi[(int64_t)(j + 3) * lw], yc[j + 3], a3);
        }
        for (; j < r3; ++j) a0 = fma(gi[(int64_t)j * lw], yc[j], a0);
        const double v = -((a0 + a1) + (a2 + a3));
        W[(int64_t)c * lw + k3 + i] = v;
        W[(int64_t)(k3 + i) * lw + c] = v;
    }
    __syncthreads();
    // Sigma_CC(a, b), a >= b: sum_{c >= a} Z(c, a) Z(c, b) - sum_i Y(i, a) Sigma_RC(i, b)
    for (int e = tid; e < k3 * k3; e += kT) {
        const int a = e % k3, b = e / k3;
        if (a < b) continue;
        const double* xa = X + (int64_t)a * lx;
        const double* xb = X + (int64_t)b * lx;
        const double* wb = W + (int64_t)b * lw;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int c = a;
        for (; c + 3 < k3; c += 4) {
            a0 = fma(xa[c], xb[c], a0);
            a1 = fma(xa[c + 1], xb[c + 1], a1);
            a2 = fma(xa[c + 2], xb[c + 2], a2);
            a3 = fma(xa[c + 3], xb[c + 3], a3);
        }
        for (; c < k3; ++c) a0 = fma(xa[c], xb[c], a0);
        double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
        c = k3;
        for (; c + 3 < m3; c += 4) {
            b0 = fma(xa[c], wb[c], b0);
            b1 = fma(xa[c + 1], wb[c + 1], b1);
            b2 = fma(xa[c + 2], wb[c + 2], b2);
            b3 = fma(xa[c + 3], wb[c + 3], b3);
        }
        for (; c < m3; ++c) b0 = fma(xa[c], wb[c], b0);
        const double v = ((a0 + a1) + (a2 + a3)) - ((b0 + b1) + (b2 + b3));
        W[(int64_t)b * lw + a] = v;
        W[(int64_t)a * lw + b] = v;
    }
    if (lds) {
        __syncthreads();
        for (int e = tid; e < m3 * m3; e += kT) {
            const int i = e % m3, j = e / m3;
            Sg[e] = W[j * lw + i];
        }
    }
}

// the requested 3x3 blocks out of the Sigma buffer, row-major: block q is at off (its (0, 0)
// element) with leading dimension ld
__global__ __launch_bounds__(256) void chol_selinv_pick(const SelPick* __restrict__ picks, int64_t n,
                                                        const double* __restrict__ sel, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 9 * n) return;
    const SelPick p = picks[e / 9];
    const int ii = (int)(e % 9) / 3, jj = (int)(e % 3);
    out[e] = sel[p.off + (int64_t)jj * p.ld + ii];
}

// ---- joint marginals: blocks of Sigma outside L's pattern (any node pair) ----
// With P H P^T = L L^T, Sigma(i, j) = W_i^T W_j, W_q = L^-1 E_q (E_q: node q's three unit columns).
// W_q is nonzero only on the pivot rows of the fronts between q's own and the root of its tree, so
// it takes one forward substitution along one root path -- the multifrontal forward solve's
// hand-over, restricted to that path -- and no backward solve.
//
// chol_path_forward: one workgroup per queried node (every gridDim.x-th query).  It carries a
// (front rows x 3) right-hand side: the identity at q's three pivot scalars in its own front.  Per
// front, kPB pivot columns at a time: the diagonal block goes to LDS, one thread per right-hand side
// substitutes through it (rows in registers, four accumulators per row: a dependent fp64 chain),
// then one thread per row below -- the rest of the pivot rows and the update rows -- subtracts the
// block's columns times the new values.  The pivot rows w_C go to the query's slice of W, the update
// rows through relmap into the parent's (zeroed) vector.  L is read from the fronts as
// chol_selinv_level reads it (column-major, leading dimension 3 (k + r), L11 above L21; the fused
// and the level factorization leave the same, and opts.solve_inv_cols puts L11^-1 in a buffer of
// its own).  The two vectors ([3][ldv] each) are in LDS when they fit kPathLds, in this
// workgroup's slice of `work` otherwise.  Every element is one thread's sum in a fixed order.
__global__ __launch_bounds__(kT) void chol_path_forward(const PathQuery* __restrict__ queries, int64_t nq,
                                                        const SnDev* __restrict__ sns, const int32_t* __restrict__ relmap,
                                                        const double* __restrict__ fronts, double* __restrict__ W,
                                                        double* work, int ldv, int in_lds) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double s_d[kPB * kPB];   // the diagonal block, column-major
    __shared__ double s_rd[kPB];        // 1 / its diagonal
    __shared__ double s_w[3 * kPB];     // the block's new values, per right-hand side
    const int tid = threadIdx.x;
    double* v0 = in_lds ? sm : work + (int64_t)blockIdx.x * 6 * ldv;
    for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        double* cur = v0;
        double* nxt = v0 + 3 * ldv;
        const PathQuery Q = queries[q];
        SnDev S = sns[Q.sn];
        int64_t wo = Q.w_off;
        {
            const int m3 = 3 * (S.k + S.r);
            for (int e = tid; e < 3 * m3; e += kT) {
                const int a = e / m3, i = e % m3;
                cur[a * ldv + i] = i == Q.row + a ? 1.0 : 0.0;
            }
        }
        for (;;) {
            const int k3 = 3 * S.k, r3 = 3 * S.r, m3 = k3 + r3;
            const double* F = fronts + S.front_off;
            for (int j0 = 0; j0 < k3; j0 += kPB) {
                const int nb = min(kPB, k3 - j0);
                for (int e = tid; e < nb * nb; e += kT) {
                    const int jj = e % nb, cc = e / nb;
                    if (jj >= cc) s_d[cc * kPB + jj] = F[(int64_t)(j0 + cc) * m3 + j0 + jj];
                }
                if (tid < nb) s_rd[tid] = 1.0 / F[(int64_t)(j0 + tid) * m3 + j0 + tid];
                __syncthreads();   // (also: the previous block's row updates are in cur)
                if (tid < 3) {
                    double* x = cur + tid * ldv + j0;
                    double b[kPB], w[kPB];
#pragma unroll
                    for (int jj = 0; jj < kPB; ++jj) b[jj] = jj < nb ? x[jj] : 0.0;
#pragma unroll
                    for (int jj = 0; jj < kPB; ++jj) {
                        if (jj < nb) {
                            double a4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int cc = 0; cc < jj; ++cc) a4[cc & 3] = fma(s_d[cc * kPB + jj], w[cc], a4[cc & 3]);
                            w[jj] = (b[jj] - ((a4[0] + a4[1]) + (a4[2] + a4[3]))) * s_rd[jj];
                            x[jj] = w[jj];
                            s_w[tid * kPB + jj] = w[jj];
                        }
                    }
                }
                __syncthreads();
                for (int i = j0 + nb + tid; i < m3; i += kT) {
                    double a4[3][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
                    const double* li = F + (int64_t)j0 * m3 + i;
#pragma unroll 4
                    for (int cc = 0; cc < nb; ++cc) {
                        const double l = li[(int64_t)cc * m3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) a4[a][cc & 3] = fma(l, s_w[a * kPB + cc], a4[a][cc & 3]);
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) cur[a * ldv + i] -= (a4[a][0] + a4[a][1]) + (a4[a][2] + a4[a][3]);
                }
                // (the next block's staging rewrites s_d and s_rd, which only the substitution read)
            }
            __syncthreads();
            for (int e = tid; e < 3 * k3; e += kT) W[wo + e] = cur[(e % 3) * ldv + e / 3];
            wo += 3 * k3;
            if (S.parent < 0) break;
            const SnDev Pn = sns[S.parent];
            const int mp3 = 3 * (Pn.k + Pn.r);
            for (int e = tid; e < 3 * mp3; e += kT) nxt[(e / mp3) * ldv + e % mp3] = 0.0;
            __syncthreads();
            const int32_t* rm = relmap + S.rows_off;
            for (int e = tid; e < 3 * r3; e += kT) {
                const int a = e / r3, t = e % r3;
                nxt[a * ldv + 3 * rm[t / 3] + t % 3] = cur[a * ldv + k3 + t];
            }
            __syncthreads();
            double* t = cur;
            cur = nxt;
            nxt = t;
            S = Pn;
        }
        __syncthreads();   // (the next query starts in v0)
    }
}

// chol_path_dot: one wave per requested block.  Lane l sums the scalars l, l + 64, ... of the two
// suffixes' nine products in order, then a fixed xor tree over the 64 lanes; an empty suffix (two
// trees of the forest) gives exactly 0.  The block and / or its transpose are stored (PathPair).
__global__ __launch_bounds__(256) void chol_path_dot(const PathPair* __restrict__ pairs, int64_t n,
                                                     const double* __restrict__ W, double* __restrict__ out, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;   // (whole wave)
    const PathPair P = pairs[p];
    const double* A = W + P.a;
    const double* B = W + P.b;
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = lane; t < P.len; t += 64) {
        const double a0 = A[3 * (int64_t)t], a1 = A[3 * (int64_t)t + 1], a2 = A[3 * (int64_t)t + 2];
        const double b0 = B[3 * (int64_t)t], b1 = B[3 * (int64_t)t + 1], b2 = B[3 * (int64_t)t + 2];
        s[0] = fma(a0, b0, s[0]); s[1] = fma(a0, b1, s[1]); s[2] = fma(a0, b2, s[2]);
        s[3] = fma(a1, b0, s[3]); s[4] = fma(a1, b1, s[4]); s[5] = fma(a1, b2, s[5]);
        s[6] = fma(a2, b0, s[6]); s[7] = fma(a2, b1, s[7]); s[8] = fma(a2, b2, s[8]);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e)
        for (int off = 32; off >= 1; off >>= 1) s[e] += __shfl_xor(s[e], off, 64);
    // (every lane holds the sums; lane e stores element e)
    double v = s[0];
#pragma unroll
    for (int e = 1; e < 9; ++e)
        if (lane == e) v = s[e];
    if (lane < 9) {
        const int r = lane / 3, c = lane % 3;
        if (P.o >= 0) out[P.o + r * ld + c] = v;
        if (P.ot >= 0) out[P.ot + c * ld + r] = v;
    }
}

// ---- selected inverse: host side ----
// the Sigma buffer, the work buffer and the lists of the current analysis (once per analysis)
int selinv_prepare(CholDev* c, hipStream_t st) {
    const dpg_chol_sym& S = c->sym;
    const size_t total = (size_t)S.front_off[(size_t)S.ns];
    if (c->sel_gen == c->build_gen && c->sel.p && total <= c->sel.cap) return DPG_OK;
    // (an earlier request's kernels may still read what is rebuilt here)
    if (hipStreamSynchronize(st) != hipSuccess) return DPG_ERR_HIP;
    const int32_t ns = S.ns;
    std::vector<int64_t> woff((size_t)ns);
    c->sel_lds.assign((size_t)S.n_levels, 0);
    int64_t wtot = 0;
    for (int32_t s = 0; s < ns; ++s) {
        const int k3 = 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]);
        const int m3 = k3 + 3 * (int)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
        if (k3 > 384) return DPG_ERR_SIZE;   // (the kernel's table of diagonal reciprocals)
        woff[(size_t)s] = wtot;
        const int need = sel_lds_doubles(m3, k3);
        if (need <= kSelLds) {
            size_t& l = c->sel_lds[(size_t)S.sn_level[(size_t)s]];
            l = std::max(l, sizeof(double) * (size_t)need);
        } else {
            wtot += (int64_t)m3 * k3;
        }
    }
    const size_t lb = sizeof(int64_t) * (size_t)ns + sizeof(int32_t) * (size_t)ns;
    if (c->sel.reserve_amortised(total) || c->sel_work.reserve_amortised((size_t)wtot) || c->sel_lists.reserve_amortised(lb))
        return DPG_ERR_HIP;
    if (hipMemcpy(c->sel_lists.p, woff.data(), sizeof(int64_t) * (size_t)ns, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->sel_lists.p + sizeof(int64_t) * (size_t)ns, S.level_list.data(), sizeof(int32_t) * (size_t)ns,
                  hipMemcpyHostToDevice) != hipSuccess)
        return DPG_ERR_HIP;
    c->sel_gen = c->build_gen;
    return DPG_OK;
}

// level_ms (may be NULL): the time of each level's launch, roots' level first, from HIP events
int selinv_run(CholDev* c, hipStream_t st, float* level_ms, int cap) {
    if (!c || !c->has_factor) return DPG_ERR_STATE;
    const int rc = selinv_prepare(c, st);
    if (rc) return rc;
    const dpg_chol_sym& S = c->sym;
    const int64_t* woff = reinterpret_cast<const int64_t*>(c->sel_lists.p);
    const int32_t* list = reinterpret_cast<const int32_t*>(c->sel_lists.p + sizeof(int64_t) * (size_t)S.ns);
    const bool timed = level_ms != nullptr;
    if (timed) {
        while ((int32_t)c->sel_ev.size() < S.n_levels + 1) {
            DevEvent e;
            if (e.ensure(hipEventDefault)) return DPG_ERR_HIP;
            c->sel_ev.push_back(std::move(e));
        }
        if (hipEventRecord(c->sel_ev[0].e, st) != hipSuccess) return DPG_ERR_HIP;
    }
    for (int32_t l = S.n_levels - 1, q = 1; l >= 0; --l, ++q) {
        const int32_t b = S.level_ptr[(size_t)l], n = S.level_ptr[(size_t)l + 1] - b;
        if (n > 0)
            hipLaunchKernelGGL(chol_selinv_level, dim3((unsigned)n), dim3(kT), c->sel_lds[(size_t)l], st, list + b, c->sns,
                               c->relmap, woff, c->fronts.p, c->sel.p, c->sel_work.p);
        if (timed && hipEventRecord(c->sel_ev[(size_t)q].e, st) != hipSuccess) return DPG_ERR_HIP;
    }
    if (hipGetLastError() != hipSuccess) return DPG_ERR_HIP;
    if (timed) {
        if (hipEventSynchronize(c->sel_ev[(size_t)S.n_levels].e) != hipSuccess) return DPG_ERR_HIP;
        for (int32_t q = 0; q < S.n_levels && q < cap; ++q)
            if (hipEventElapsedTime(level_ms + q, c->sel_ev[(size_t)q].e, c->sel_ev[(size_t)q + 1].e) != hipSuccess)
                return DPG_ERR_HIP;
    }
    return DPG_OK;
}

// block (row node i, column node j) of Sigma in the front of the earlier of the two; false when
// the block is outside L's pattern
bool sel_locate(const dpg_chol_sym& S, int32_t i, int32_t j, SelPick* p) {
    const int32_t pi = S.pos[(size_t)i], pj = S.pos[(size_t)j];
    const int32_t s = S.sn_of[(size_t)std::min(pi, pj)];
    const int32_t c0 = S.sn_c0[(size_t)s], k = S.sn_c0[(size_t)s + 1] - c0;
    const int32_t* rb = S.sn_rows.data() + S.sn_rows_ptr[(size_t)s];
    const int32_t r = (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
    auto local = [&](int32_t q) -> int32_t {
        if (q < c0 + k) return q - c0;
        const int32_t* it = std::lower_bound(rb, rb + r, q);
        return it != rb + r && *it == q ? k + (int32_t)(it - rb) : -1;
    };
    const int32_t li = local(pi), lj = local(pj);
    if (li < 0 || lj < 0) return false;
    const int32_t m3 = 3 * (k + r);
    p->off = S.front_off[(size_t)s] + (int64_t)(3 * lj) * m3 + 3 * li;
    p->ld = m3;
    p->pad = 0;
    return true;
}

// the end of a request: the status word and the result (tmp.size() doubles at dev) to the host;
// DPG_ERR_NUMERIC on a raised status or any NaN -- the caller copies tmp out only after DPG_OK
int fetch_checked(CholDev* c, hipStream_t st, const double* dev, std::vector<double>& tmp) {
    int32_t status = 0;
    if (hipMemcpyAsync(&status, c->status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        (!tmp.empty() && hipMemcpyAsync(tmp.data(), dev, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return DPG_ERR_HIP;
    if (status != 0) return DPG_ERR_NUMERIC;
    for (double v : tmp)
        if (!(v == v)) return DPG_ERR_NUMERIC;
    return DPG_OK;
}
}  // namespace

extern "C" int dpg_chol_selinv(void* h, void* stream) {
    return selinv_run(reinterpret_cast<CholDev*>(h), reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int dpg_chol_selinv_timed(void* h, void* stream, float* level_ms, int cap) {
    return selinv_run(reinterpret_cast<CholDev*>(h), reinterpret_cast<hipStream_t>(stream), level_ms, cap);
}

// host only: the nodes are in range and every pair's block lies in L's pattern (nodes == NULL:
// all of them in order, n = the graph's size)
extern "C" int dpg_chol_selinv_check(void* h, const int32_t* nodes, int64_t n, const int32_t* pairs, int64_t n_pairs) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    if (!c) return DPG_ERR_STATE;
    const dpg_chol_sym& S = c->sym;
    if (n < 0 || n_pairs < 0 || (!nodes && n != 0 && n != S.n) || (n_pairs > 0 && !pairs)) return DPG_ERR_ARG;
    for (int64_t q = 0; nodes && q < n; ++q)
        if (nodes[q] < 0 || nodes[q] >= S.n) return DPG_ERR_ARG;
    SelPick p;
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || i >= S.n || j < 0 || j >= S.n || !sel_locate(S, i, j, &p)) return DPG_ERR_ARG;
    }
    return DPG_OK;
}

extern "C" int dpg_chol_selinv_gather(void* h, const int32_t* nodes, int64_t n, const int32_t* pairs, int64_t n_pairs,
                                      double* out_dev, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    const int rc = dpg_chol_selinv_check(h, nodes, n, pairs, n_pairs);
    if (rc) return rc;
    if (!c->sel.p || c->sel_gen != c->build_gen) return DPG_ERR_STATE;
    const int64_t nb = n + n_pairs;
    if (nb == 0) return DPG_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dpg_chol_sym& S = c->sym;
    std::vector<SelPick>& P = c->h_picks;
    P.resize((size_t)nb);
    for (int64_t q = 0; q < n; ++q) {
        const int32_t v = nodes ? nodes[q] : (int32_t)q;
        sel_locate(S, v, v, &P[(size_t)q]);
    }
    for (int64_t q = 0; q < n_pairs; ++q) sel_locate(S, pairs[2 * q], pairs[2 * q + 1], &P[(size_t)(n + q)]);
    // (the list is rewritten per request: the previous request's kernel must be done with it)
    if (hipStreamSynchronize(st) != hipSuccess || c->sel_picks.reserve_amortised((size_t)nb) ||
        hipMemcpy(c->sel_picks.p, P.data(), sizeof(SelPick) * (size_t)nb, hipMemcpyHostToDevice) != hipSuccess)
        return DPG_ERR_HIP;
    hipLaunchKernelGGL(chol_selinv_pick, dim3((unsigned)((9 * nb + 255) / 256)), dim3(256), 0, st, c->sel_picks.p, nb, c->sel.p,
                       out_dev);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// Sigma from the factor in place, then the requested blocks to the host (nodes first, then pairs;
// [n + n_pairs][9] row-major).  Nothing is written to host_out unless everything succeeded.
extern "C" int dpg_chol_marginals(void* h, const int32_t* nodes, int64_t n, const int32_t* pairs, int64_t n_pairs,
                                  double* host_out, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    int rc = dpg_chol_selinv_check(h, nodes, n, pairs, n_pairs);
    if (rc) return rc;
    const int64_t nb = n + n_pairs;
    if ((rc = dpg_chol_selinv(h, stream))) return rc;
    if (c->sel_out.reserve_amortised((size_t)(9 * nb))) return DPG_ERR_HIP;
    if ((rc = dpg_chol_selinv_gather(h, nodes, n, pairs, n_pairs, c->sel_out.p, stream))) return rc;
    std::vector<double> tmp((size_t)(9 * nb));
    if ((rc = fetch_checked(c, reinterpret_cast<hipStream_t>(stream), c->sel_out.p, tmp))) return rc;
    if (nb > 0) memcpy(host_out, tmp.data(), sizeof(double) * 9 * (size_t)nb);
    return DPG_OK;
}

extern "C" int64_t dpg_chol_selinv_bytes(void* h) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    return c ? (int64_t)(sizeof(double) * (c->sel.cap + c->sel_work.cap)) : 0;
}

// ---- joint marginals: host side ----
// Blocks of Sigma for any nodes from the factor h holds now (only read): by_nodes = 0 -- idx is
// pairs[n][2] and host_out[n][9] gets Sigma(i, j) row-major; by_nodes = 1 -- idx is nodes[n] and
// host_out[3n][3n] gets their joint covariance.  ms (may be NULL): the path solve's and the dot
// kernel's time from HIP events.  Nothing is written to host_out unless everything succeeded.
extern "C" int dpg_chol_joint(void* h, int by_nodes, const int32_t* idx, int64_t n, double* host_out, void* stream,
                              float* ms) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c) return DPG_ERR_STATE;
    const dpg_chol_sym& S = c->sym;
    if (n < 0 || (n > 0 && (!idx || !host_out))) return DPG_ERR_ARG;
    for (int64_t q = 0, e = by_nodes ? n : 2 * n; q < e; ++q)
        if (idx[q] < 0 || idx[q] >= S.n) return DPG_ERR_ARG;
    if (!c->has_factor) return DPG_ERR_STATE;
    if (ms) ms[0] = ms[1] = 0.f;
    if (n == 0) return DPG_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    JointPlan& J = c->jplan;
    if (by_nodes) dpg_chol_plan_joint_nodes(J, S, idx, n);
    else dpg_chol_plan_joint_pairs(J, S, idx, n);
    const int64_t nq = (int64_t)J.queries.size(), np = (int64_t)J.pairs.size();
    const int ldv = path_ldv(S.max_front);
    const bool in_lds = path_in_lds(S.max_front);
    const unsigned grid = (unsigned)std::min<int64_t>(nq, kPathGrid);
    const size_t pb = sizeof(PathPair) * (size_t)np, qb = sizeof(PathQuery) * (size_t)nq;
    // (the lists are rewritten per request: an earlier request's kernels must be done with them)
    if (hipStreamSynchronize(st) != hipSuccess || c->jt_w.reserve_amortised((size_t)J.w_total) ||
        c->jt_work.reserve_amortised(in_lds ? 1 : (size_t)grid * 6 * (size_t)ldv) ||
        c->jt_out.reserve_amortised((size_t)J.out_total) || c->jt_lists.reserve_amortised(pb + qb) ||
        hipMemcpy(c->jt_lists.p, J.pairs.data(), pb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->jt_lists.p + pb, J.queries.data(), qb, hipMemcpyHostToDevice) != hipSuccess)
        return DPG_ERR_HIP;
    if (ms)
        for (DevEvent& e : c->jt_ev)
            if (e.ensure(hipEventDefault)) return DPG_ERR_HIP;
    const PathPair* pairs = reinterpret_cast<const PathPair*>(c->jt_lists.p);
    const PathQuery* queries = reinterpret_cast<const PathQuery*>(c->jt_lists.p + pb);
    if (ms && hipEventRecord(c->jt_ev[0].e, st) != hipSuccess) return DPG_ERR_HIP;
    hipLaunchKernelGGL(chol_path_forward, dim3(grid), dim3(kT), in_lds ? sizeof(double) * 6 * (size_t)ldv : 0, st, queries, nq,
                       c->sns, c->relmap, c->fronts.p, c->jt_w.p, c->jt_work.p, ldv, in_lds ? 1 : 0);
    if (ms && hipEventRecord(c->jt_ev[1].e, st) != hipSuccess) return DPG_ERR_HIP;
    hipLaunchKernelGGL(chol_path_dot, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st, pairs, np, c->jt_w.p, c->jt_out.p,
                       (int64_t)J.ld);
    if (ms && hipEventRecord(c->jt_ev[2].e, st) != hipSuccess) return DPG_ERR_HIP;
    if (hipGetLastError() != hipSuccess) return DPG_ERR_HIP;
    std::vector<double> tmp((size_t)J.out_total);
    const int rc = fetch_checked(c, st, c->jt_out.p, tmp);
    if (rc) return rc;
    if (ms && (hipEventElapsedTime(ms, c->jt_ev[0].e, c->jt_ev[1].e) != hipSuccess ||
               hipEventElapsedTime(ms + 1, c->jt_ev[1].e, c->jt_ev[2].e) != hipSuccess))
        return DPG_ERR_HIP;
    memcpy(host_out, tmp.data(), sizeof(double) * tmp.size());
    return DPG_OK;
}

// the longest root path among the analysis's nodes: {fronts, pivot scalars}
extern "C" void dpg_chol_path_stats(void* h, int64_t out[2]) {
    const dpg_chol_sym& S = reinterpret_cast<CholDev*>(h)->sym;
    out[0] = out[1] = 0;
    for (int32_t s0 = 0; s0 < S.ns; ++s0) {
        int64_t nf = 0, len = 0;
        for (int32_t s = s0; s >= 0; s = S.sn_parent[(size_t)s]) {
            ++nf;
            len += 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]);
        }
        out[0] = std::max(out[0], nf);
        out[1] = std::max(out[1], len);
    }
}
