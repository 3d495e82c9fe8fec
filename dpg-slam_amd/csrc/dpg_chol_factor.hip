// dpg_chol_factor.hip -- the fused factorization + forward solve of the GPU Cholesky (ONE launch,
// fronts as a DAG), and the run copies of the partial refactorization that keeps fronts of the
// last one.  fp64 throughout, explicit fma in the inner products.
#include "dpg_chol_dev.h"

using namespace dpg_chol;

// per front of the fused kernel: [front][0 claim, 1 children ready, 2 assembled, 3 factored, 4 done]
#define FT_MARK(s, k) DPG_STAMP(threadIdx.x == 0 && (s) < 16384, g_front[(s) * 8 + (k)])
// per panel of a large front: [front][panel][0 wake, 1 loaded, 2 tile updated, 3 factored, 4 published]
#define PN_MARK(s, p, k) DPG_STAMP(threadIdx.x == 0 && (s) < 16384 && (p) < 16, g_panel[((s) * 16 + (p)) * 8 + (k)])
#ifdef DPG_CHOL_TIMING
__device__ unsigned long long g_front[16384 * 8], g_panel[16384 * 16 * 8];
extern "C" int dpg_chol_front_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_front), sizeof(unsigned long long) * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_panel_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_panel), sizeof(unsigned long long) * 16 * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif

namespace {
// One 512-thread workgroup per front, claimed in topological order (as the solves' fronts).  A
// front waits for its children, then
//   assembles itself column tile by column tile in LDS (H blocks + children's update matrices,
//     child by child: fixed summation order),
//   factors its k3 pivot columns right-looking by kFNB-column panels: the panel is staged in LDS,
//     wave 0 factors its top w x w block with the rows in registers (rsq + Newton, 3x3-block steps,
//     wave-synchronous, no workgroup barrier), every other row solves against it independently
//     (one row per thread, L_top broadcast from LDS), then the whole workgroup applies the rank-w
//     update to the trailing lower triangle in 64x64 tiles (4x4 register tile per thread),
//   runs its part of the forward solve L y = -g while its L is hot (children's pending row updates
//     gathered in child order, diagonal blocks by one wave, L21 y handed to the parent),
//   and signals its parent.
// Hand-off (dpg_chol_dev.h): everything another workgroup reads -- the update matrix (columns >= k3)
// and the pending row updates -- is stored write-through and read back with sc1 loads.
// (kFT threads, kFNB-column panels, the kSmall / kMaxCh rule, teams of up to kGmax and the LDS
// carve fused_rp / kFScr / fused_lds_doubles: dpg_chol_plan.h)
constexpr int kPF = (kSmall * (kSmall + 1) / 2 + kFT - 1) / kFT;   // per-thread prefetch slots per child
constexpr int kPFL = 4;      // large fronts: entries in flight per thread in the extend-add / publish rounds

// packed lower triangle of an n x n matrix, column-major: entry e -> (row i, column j), i >= j
__device__ __forceinline__ void tri_ij(int e, int n, int& i, int& j) {
    const float b = 2.0f * (float)n + 1.0f;
    int jj = (int)((b - sqrtf(b * b - 8.0f * (float)e)) * 0.5f);
    jj = max(0, min(jj, n - 1));
    while (jj > 0 && jj * n - jj * (jj - 1) / 2 > e) --jj;
    while (jj + 1 < n && (jj + 1) * n - (jj + 1) * jj / 2 <= e) ++jj;
    j = jj;
    i = jj + e - (jj * n - jj * (jj - 1) / 2);
}

// A front of at most kSmall rows, entirely in LDS: H blocks and the right-hand side are scattered
// while the children are still running; after the wait the children's update matrices and pending
// row updates arrive through ONE pipelined round of sc1 loads (child c + 1 in flight while child c
// is added; child order fixes the summation order); the factorization runs by 3x3 block columns
// with the right-hand side as an extra column (so the forward solve is folded in); the finished
// L columns, y, the update matrix (sc1) and the pending row updates (sc1) go out once.
__device__ __forceinline__ void small_front(int s, const SnDev& S, int32_t* sync, int32_t* status, const SnDev* __restrict__ sns,
                            const OEnt* __restrict__ omap, const int32_t* __restrict__ relmap,
                            const int32_t* __restrict__ child_list, const double* __restrict__ hb,
                            const double* __restrict__ g, const int32_t* __restrict__ perm, double* fronts,
                            double* __restrict__ ysol, double* acc, double* sm) {
    const int tid = threadIdx.x;
    const int k3 = 3 * S.k, r3 = 3 * S.r, m3 = k3 + r3;
    double* F = fronts + S.front_off;
    double* A = sm;                                           // [m3][m3] column-major
    double* bv = A + m3 * m3;                                 // [m3] right-hand side column
    ChMeta* chm = reinterpret_cast<ChMeta*>(bv + m3);   // m3 (m3 + 1) doubles: 16-B aligned
    int32_t* crm = reinterpret_cast<int32_t*>(chm + kMaxCh);  // [kMaxCh][kSmall / 3] child relmaps
    const int nch = S.nchild;
    // ---- before the wait: everything that does not come from the children
    for (int e = tid; e < m3 * m3; e += kFT) A[e] = 0.0;
    for (int t = tid; t < m3; t += kFT) bv[t] = t < k3 ? -g[3 * perm[S.c0 + t / 3] + t % 3] : 0.0;
    if (tid < nch) {
        const SnDev C = sns[child_list[S.child_off + tid]];
        chm[tid] = ChMeta{C.front_off, C.acc_off, C.rows_off, C.k, C.r};
        for (int q = 0; q < C.r; ++q) crm[tid * (kSmall / 3) + q] = relmap[C.rows_off + q];
    }
    __syncthreads();
    for (int q = tid; q < S.omap_n * 9; q += kFT) {
        const OEnt o = omap[S.omap_off + q / 9];
        const int ii = (q % 9) / 3, jj = q % 3;
        const int row = 3 * o.a + ii, col = 3 * o.b + jj;
        if (row < col) continue;
        const double* B = hb + 9 * (int64_t)o.u;
        A[col * m3 + row] = o.tr ? B[3 * jj + ii] : B[3 * ii + jj];
    }
    if (nch > 0) {
        if (tid == 0) wait_geq_sc1(sync + s, S.need, status);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    FT_MARK(s, 1);
    // ---- children: update matrices (packed lower triangles) + pending row updates
    auto load_child = [&](int ci, double (&v)[kPF], double& va) {
        const ChMeta C = chm[ci];
        const int n = 3 * C.r, tri = n * (n + 1) / 2, m3c = 3 * (C.k + C.r), k3c = 3 * C.k;
        double* Fc = fronts + C.front_off + (int64_t)k3c * m3c + k3c;
#pragma unroll
        for (int q = 0; q < kPF; ++q) {
            const int e = tid + kFT * q;
            v[q] = 0.0;
            if (e < tri) {
                int i, j;
                tri_ij(e, n, i, j);
                v[q] = ld_agent(Fc + (int64_t)j * m3c + i);
            }
        }
        va = tid < n ? ld_agent(acc + C.acc_off + tid) : 0.0;
    };
    auto add_child = [&](int ci, const double (&v)[kPF], double va) {
        const ChMeta C = chm[ci];
        const int n = 3 * C.r, tri = n * (n + 1) / 2;
        const int32_t* rm = crm + ci * (kSmall / 3);
#pragma unroll
        for (int q = 0; q < kPF; ++q) {
            const int e = tid + kFT * q;
            if (e < tri) {
                int i, j;
                tri_ij(e, n, i, j);
                const int pj = 3 * rm[j / 3] + j % 3, pi = 3 * rm[i / 3] + i % 3;
                A[pj * m3 + pi] += v[q];
            }
        }
        if (tid < n) bv[3 * rm[tid / 3] + tid % 3] -= va;
    };
    if (nch > 0) {
        double va_[kPF], vb_[kPF], aa = 0.0, ab = 0.0;
        load_child(0, va_, aa);
        for (int ci = 0; ci < nch; ci += 2) {
            if (ci + 1 < nch) load_child(ci + 1, vb_, ab);
            add_child(ci, va_, aa);
            __syncthreads();
            if (ci + 1 < nch) {
                if (ci + 2 < nch) load_child(ci + 2, va_, aa);
                add_child(ci + 1, vb_, ab);
                __syncthreads();
            }
        }
    }
    FT_MARK(s, 2);
    // ---- factorization by 3x3 block columns, right-hand side as column m3
    bool bad = false;
    for (int c0 = 0; c0 < k3; c0 += 3) {
        const double* C0 = A + c0 * m3;
        const double* C1 = C0 + m3;
        const double* C2 = C1 + m3;
        double d00 = C0[c0], d10 = C0[c0 + 1], d20 = C0[c0 + 2], d11 = C1[c0 + 1], d21 = C1[c0 + 2], d22 = C2[c0 + 2];
        if (!(d00 > 0.0)) { bad = true; d00 = 1.0; }
        const double i00 = rsqrt_nr(d00), l00 = d00 * i00;
        const double l10 = d10 * i00, l20 = d20 * i00;
        double e11 = d11 - l10 * l10;
        if (!(e11 > 0.0)) { bad = true; e11 = 1.0; }
        const double i11 = rsqrt_nr(e11), l11 = e11 * i11;
        const double l21 = (d21 - l20 * l10) * i11;
        double e22 = d22 - l20 * l20 - l21 * l21;
        if (!(e22 > 0.0)) { bad = true; e22 = 1.0; }
        const double i22 = rsqrt_nr(e22), l22 = e22 * i22;
        const double y0 = bv[c0] * i00;
        const double y1 = (bv[c0 + 1] - l10 * y0) * i11;
        const double y2 = (bv[c0 + 2] - l20 * y0 - l21 * y1) * i22;
        for (int i = c0 + 3 + tid; i < m3; i += kFT) {
            const double x0 = C0[i] * i00;
            const double x1 = (C1[i] - x0 * l10) * i11;
            const double x2 = (C2[i] - x0 * l20 - x1 * l21) * i22;
            A[c0 * m3 + i] = x0;
            A[(c0 + 1) * m3 + i] = x1;
            A[(c0 + 2) * m3 + i] = x2;
            bv[i] -= x0 * y0 + x1 * y1 + x2 * y2;
        }
        __syncthreads();
        if (tid == 0) {
            A[c0 * m3 + c0] = l00; A[c0 * m3 + c0 + 1] = l10; A[c0 * m3 + c0 + 2] = l20;
            A[(c0 + 1) * m3 + c0 + 1] = l11; A[(c0 + 1) * m3 + c0 + 2] = l21; A[(c0 + 2) * m3 + c0 + 2] = l22;
            bv[c0] = y0; bv[c0 + 1] = y1; bv[c0 + 2] = y2;
        }
        const int b0 = c0 + 3, nr = m3 - b0;
        for (int e = tid; e < nr * nr; e += kFT) {
            const int l = b0 + e / nr, i = b0 + e % nr;
            if (i < l) continue;
            double v = A[l * m3 + i];
            v = fma(-C0[i], C0[l], v);
            v = fma(-C1[i], C1[l], v);
            v = fma(-C2[i], C2[l], v);
            A[l * m3 + i] = v;
        }
        __syncthreads();
    }
    if (bad && tid == 0) atomicExch(status, 1);
    FT_MARK(s, 3);
    // ---- out: L columns + y (read by the backward solve, next launch), update matrix + pending (sc1)
    for (int e = tid; e < k3 * m3; e += kFT) {
        const int j = e / m3, i = e - j * m3;
        if (i >= j) F[(int64_t)j * m3 + i] = A[e];
    }
    for (int t = tid; t < k3; t += kFT) ysol[3 * (int64_t)S.c0 + t] = bv[t];
    if (S.parent >= 0) {   // the update matrix: 16-B sc1 stores of the aligned pairs over its columns
        const auto rs = front_rsrc(F, m3);
        const int npc = (r3 + 2) >> 1;
        for (int e = tid; e < r3 * npc; e += kFT) {
            const int jj = e / npc, k = e - jj * npc, j = k3 + jj;
            const uint32_t a = (uint32_t)(j * m3 + k3);
            const int i0 = 2 * k - (int)(a & 1u);   // rows k3 + i0, k3 + i0 + 1
            if (i0 + 1 < jj || i0 >= r3) continue;
            const double* Aj = A + j * m3 + k3;
            st2_sc1(rs, (a & ~1u) + 2u * k, i0 >= jj ? Aj[i0] : 0.0, i0 + 1 < r3 ? Aj[i0 + 1] : 0.0);
        }
        for (int t = tid; t < r3; t += kFT) st_agent(acc + S.acc_off + t, -bv[k3 + t]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FT_MARK(s, 4);
    if (tid == 0 && S.parent >= 0)
        __hip_atomic_fetch_add(sync + S.parent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the column tiles of a large front (large_front, below): np pivot tiles of kFNB columns, then update tiles from k3
struct Tiles {
    int k3, m3, np, nt;
    __device__ int c0(int t) const { return t < np ? kFNB * t : k3 + kFNB * (t - np); }
    __device__ int c1(int t) const { return t < np ? min(kFNB * t + kFNB, k3) : min(k3 + kFNB * (t - np + 1), m3); }
};

// The frame of pivot panel q of a large front: front columns [j0, j0 + w), rows j0 .. m3 (R of
// them).  In LDS, element (row i, column c) of the frame sits at P[c * Rp + off + i], `off` chosen
// so that the rows below the w x w top block start 32-B aligned.  Between workgroups a column goes
// as npc aligned 16-B pairs of front elements (publish_panel stores what load_panel loads).
struct PanelFrame {
    int m3, j0, w, R, off, Rp, npc;
    __device__ __forceinline__ PanelFrame(const Tiles& T, int q)
        : m3(T.m3), j0(kFNB * q), w(min(kFNB, T.k3 - j0)), R(T.m3 - j0), off((4 - (w & 3)) & 3), Rp(fused_rp(R, off)),
          npc((R + 2) >> 1) {}
    // pair e of the w * npc: its column, its first row in the frame (-1: the element before the
    // column segment) and its front element (even)
    struct Pair { int c, i0; uint32_t addr; };
    __device__ __forceinline__ Pair pair(int e) const {
        const int c = e / npc, k = e - c * npc;
        const uint32_t a = (uint32_t)((j0 + c) * m3 + j0);
        return Pair{c, 2 * k - (int)(a & 1u), (a & ~1u) + 2u * k};
    }
};

// Panel q of a large front, in LDS (P, the panel frame: column c of the tile at P[c * Rp + off + i],
// rows i >= c valid, zeros above): POTRF of the top w x w block, TRSM of the rows below, L_top
// copied back.  `scr` holds L_top, the 3x3 inverses and the POTRF column exchange.
__device__ void factor_lds(int q, int s, const Tiles& T, double* P, double* scr, bool& bad) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PanelFrame f(T, q);
    const int w = f.w, R = f.R, off = f.off, Rp = f.Rp;
    double* Lt = scr;
    double* rdg = Lt + kFNB * kFNB;
    int* flg = reinterpret_cast<int*>(rdg + 8 * (kFNB / 3));   // [kFNB / 3] step epochs (zeroed by the chain's start)
    PN_MARK(s, q, 5);
    // POTRF of the top w x w block, pipelined over the waves: wave v owns the 3x3 block column
    // 3v..3v+2 (lane = row, its three columns in registers).  It applies each earlier step's
    // update as soon as that step's columns are posted (L_top in LDS + an LDS epoch flag: a
    // wave-to-wave hand-off, no workgroup barrier per step), then factors its own 3x3 block,
    // posts its columns and raises its flag -- the chain per step is flag -> three fma ->
    // chol3 -> post.  Same arithmetic and order as a step-by-step POTRF.
    {
        const int i = lane, cv = 3 * wave, ep = q + 1;
        if (cv < w) {   // wave-uniform
            double col[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int c = cv + r;
                col[r] = (i < w && i >= c) ? P[c * Rp + off + i] : 0.0;
            }
            for (int st = 0; st < wave; ++st) {
                while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(flg + st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < ep)
                    __builtin_amdgcn_s_sleep(0);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const int c0 = 3 * st;
                const int ii = i < kFNB ? i : 0;
                const double x0 = Lt[c0 * kFNB + ii], x1 = Lt[(c0 + 1) * kFNB + ii], x2 = Lt[(c0 + 2) * kFNB + ii];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int c = cv + r;
                    const double y0 = Lt[c0 * kFNB + c], y1 = Lt[(c0 + 1) * kFNB + c], y2 = Lt[(c0 + 2) * kFNB + c];
                    const double v = fma(-x2, y2, fma(-x1, y1, fma(-x0, y0, col[r])));
                    col[r] = (i >= c && i < w) ? v : col[r];
                }
            }
            const double d00 = rdlane(col[0], cv), d10 = rdlane(col[0], cv + 1), d20 = rdlane(col[0], cv + 2);
            const double d11 = rdlane(col[1], cv + 1), d21 = rdlane(col[1], cv + 2), d22 = rdlane(col[2], cv + 2);
            const Chol3 L = chol3(d00, d10, d11, d20, d21, d22, bad);
            double x0 = col[0] * L.m00;
            double x1 = fma(col[0], L.m10, col[1] * L.m11);
            double x2 = fma(col[0], L.m20, fma(col[1], L.m21, col[2] * L.m22));
            if (i == cv) { x0 = L.l00; x1 = 0.0; x2 = 0.0; }
            else if (i == cv + 1) { x0 = L.l10; x1 = L.l11; x2 = 0.0; }
            else if (i == cv + 2) { x0 = L.l20; x1 = L.l21; x2 = L.l22; }
            if (i < kFNB) {
                Lt[cv * kFNB + i] = (i >= cv && i < w) ? x0 : 0.0;
                Lt[(cv + 1) * kFNB + i] = (i >= cv + 1 && i < w) ? x1 : 0.0;
                Lt[(cv + 2) * kFNB + i] = (i >= cv + 2 && i < w) ? x2 : 0.0;
            }
            if (i == 0) {
                double* mi = rdg + 2 * cv;   // 8 doubles per 3x3 block
                mi[0] = L.m00; mi[1] = L.m10; mi[2] = L.m11; mi[3] = L.m20; mi[4] = L.m21; mi[5] = L.m22;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (i == 0) __hip_atomic_store(flg + wave, ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (cv < kFNB) {   // a short last panel: this wave's columns are past w
            for (int r = 0; r < 3; ++r)
                if (i < kFNB) Lt[(cv + r) * kFNB + i] = 0.0;
        }
    }
    __syncthreads();
    PN_MARK(s, q, 6);
    // rows below: a L_top^T = row, one row per thread, by 3x3 blocks (x_b = a_b Minv_b^T, then the
    // later blocks of the row are updated -- all their products independent)
    for (int i = w + tid; i < R; i += kFT) {
        double a[kFNB];
#pragma unroll
        for (int c = 0; c < kFNB; ++c) a[c] = c < w ? P[c * Rp + off + i] : 0.0;
#pragma unroll
        for (int b = 0; b < kFNB; b += 3) {
            if (b < w) {
                const double* mi = rdg + 2 * b;
                const double x0 = a[b] * mi[0];
                const double x1 = fma(a[b], mi[1], a[b + 1] * mi[2]);
                const double x2 = fma(a[b], mi[3], fma(a[b + 1], mi[4], a[b + 2] * mi[5]));
                a[b] = x0; a[b + 1] = x1; a[b + 2] = x2;
#pragma unroll
                for (int cc = b + 3; cc < kFNB; ++cc)
                    a[cc] = fma(-x2, Lt[(b + 2) * kFNB + cc], fma(-x1, Lt[(b + 1) * kFNB + cc], fma(-x0, Lt[b * kFNB + cc], a[cc])));
            }
        }
#pragma unroll
        for (int c = 0; c < kFNB; ++c)
            if (c < w) P[c * Rp + off + i] = a[c];
    }
    __syncthreads();
    PN_MARK(s, q, 7);
    for (int e = tid; e < w * w; e += kFT) {
        const int c = e / w, r = e - c * w;
        if (r >= c) P[c * Rp + off + r] = Lt[c * kFNB + r];
    }
    __syncthreads();
    PN_MARK(s, q, 3);
}

// the factored panel q (LDS) -> its front columns, write-through, then the panel flag
__device__ void publish_panel(int q, int s, const Tiles& T, double* F, const double* P, int32_t* pflag) {
    const int tid = threadIdx.x;
    const PanelFrame f(T, q);
    const int R = f.R;
    const auto rs = front_rsrc(F, T.m3);
    for (int e = tid; e < f.w * f.npc; e += kFT) {
        const PanelFrame::Pair pr = f.pair(e);
        const int c = pr.c, i0 = pr.i0;
        if (i0 + 1 < c || i0 >= R) continue;   // wholly above the diagonal, or past the column
        const double* pc = P + c * f.Rp + f.off;
        st2_sc1(rs, pr.addr, i0 >= c ? pc[i0] : 0.0, i0 + 1 < R ? pc[i0 + 1] : 0.0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(pflag + s, q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    PN_MARK(s, q, 4);
}

// the pivot columns of tile p (= panel p's columns) -> LDS in the panel frame, zeros above the
// diagonal; SC1: the columns were handed off by another workgroup (sc1 loads), else plain
template <bool SC1>
__device__ void load_panel(int p, const Tiles& T, double* F, double* P) {
    const int tid = threadIdx.x;
    const PanelFrame f(T, p);
    const int j0 = f.j0, w = f.w, R = f.R, off = f.off, Rp = f.Rp;
    if (SC1) {   // 16-B sc1 loads of the aligned pairs (publish_panel's cover of each column segment)
        const auto rs = front_rsrc(F, T.m3);
        const int tot = w * f.npc;
        constexpr int kB2 = 8;
        for (int e0 = 0; e0 < tot; e0 += kFT * kB2) {
            double2 v[kB2];
#pragma unroll
            for (int q = 0; q < kB2; ++q) {
                const int e = e0 + tid + kFT * q;
                const PanelFrame::Pair pr = f.pair(e);
                v[q] = make_double2(0.0, 0.0);
                if (e < tot && pr.i0 < R && pr.i0 + 1 >= pr.c) v[q] = ld2_sc1(rs, pr.addr);
            }
#pragma unroll
            for (int q = 0; q < kB2; ++q) {
                const int e = e0 + tid + kFT * q;
                const PanelFrame::Pair pr = f.pair(e);
                const int c = pr.c, i0 = pr.i0;
                if (e < tot) {
                    double* pc = P + c * Rp + off;
                    if (i0 >= 0 && i0 < R) pc[i0] = i0 >= c ? v[q].x : 0.0;
                    if (i0 + 1 < R) pc[i0 + 1] = i0 + 1 >= c ? v[q].y : 0.0;
                }
            }
        }
        return;
    }
    constexpr int kB = 16;
    for (int e0 = 0; e0 < w * R; e0 += kFT * kB) {
        double v[kB];
#pragma unroll
        for (int q = 0; q < kB; ++q) {
            const int e = e0 + tid + kFT * q;
            const int c = e / R, i = e - c * R;
            double* a = F + (uint32_t)((j0 + c) * T.m3 + j0 + i);
            v[q] = (e < w * R && i >= c) ? (SC1 ? ld_agent(a) : *a) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kB; ++q) {
            const int e = e0 + tid + kFT * q;
            const int c = e / R, i = e - c * R;
            if (e < w * R) P[c * Rp + off + i] = v[q];
        }
    }
}

// rank-w update of tile t with panel p (in LDS), 4x4 register tiles, RMW of the owner's columns
// (WT: the results are stored write-through, the tile is handed off next; SC1: the tile was handed
// off to this workgroup, read it sc1)
template <bool WT, bool SC1 = false>
__device__ void update_tile(int t, int p, const Tiles& T, double* F, const double* P) {
    const int tid = threadIdx.x;
    const PanelFrame f(T, p);
    const int m3 = f.m3, j0 = f.j0, w = f.w, R = f.R, off = f.off, Rp = f.Rp;
    const int l0 = T.c0(t) - j0, l1 = T.c1(t) - j0;   // the tile's columns, panel frame
    const int g0 = ((l0 + off) & ~3) - off;            // 4-aligned group start (<= l0)
    const int ncg = (l1 - g0 + 3) >> 2, nrg = (R - g0 + 3) >> 2;
    for (int q = tid; q < nrg * ncg; q += kFT) {
        const int ib = g0 + 4 * (q % nrg), lb = g0 + 4 * (q / nrg);
        if (ib + 3 < lb) continue;
        double ac[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) ac[a][b] = 0.0;
#pragma unroll 1
        for (int c = 0; c < w; ++c) {
            const double2* pc = reinterpret_cast<const double2*>(P + c * Rp);
            const double2 i01 = pc[(off + ib) >> 1], i23 = pc[((off + ib) >> 1) + 1];
            const double2 l01 = pc[(off + lb) >> 1], l23 = pc[((off + lb) >> 1) + 1];
            const double vi[4] = {i01.x, i01.y, i23.x, i23.y};
            const double vl[4] = {l01.x, l01.y, l23.x, l23.y};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) ac[a][b] = fma(vi[a], vl[b], ac[a][b]);
        }
        // the tile's current values (clamped addresses: all 16 loads issue before any store)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t o = (uint32_t)((j0 + min(max(lb + b, l0), l1 - 1)) * m3 + j0);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                double* src = F + o + (uint32_t)min(ib + a, R - 1);
                ac[a][b] = (SC1 ? ld_agent(src) : *src) - ac[a][b];
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int l = lb + b;
            const uint32_t o = (uint32_t)((j0 + l) * m3 + j0);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int i = ib + a;
                if (l >= l0 && l < l1 && i < R && i >= l) {
                    if (WT) st_agent(F + o + (uint32_t)i, ac[a][b]);
                    else F[o + (uint32_t)i] = ac[a][b];
                }
            }
        }
    }
}

// the chain's own step: pivot tile p + 1 (loaded into Pn, its panel frame) -= panel p (Pc, full
// width) restricted to the tile; LDS to LDS, 4x4 register tiles
__device__ void update_next_lds(int p, const Tiles& T, const double* Pc, double* Pn) {
    const int tid = threadIdx.x;
    const int j0 = kFNB * p, R = T.m3 - j0, Rp = fused_rp(R, 0);   // panel p is full: off 0
    // panel p + 1's frame relative to panel p's (PanelFrame(T, p + 1), spelled from R)
    const int j1 = j0 + kFNB, w1 = min(kFNB, T.k3 - j1), R1 = R - kFNB;
    const int off1 = (4 - (w1 & 3)) & 3, Rp1 = fused_rp(R1, off1);
    const int ncg = (w1 + 3) >> 2, nrg = (R1 + 3) >> 2;
    for (int q = tid; q < nrg * ncg; q += kFT) {
        const int ib = 4 * (q % nrg), lb = 4 * (q / nrg);
        if (ib + 3 < lb) continue;
        double ac[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) ac[a][b] = 0.0;
#pragma unroll 2
        for (int c = 0; c < kFNB; ++c) {
            const double2* pc = reinterpret_cast<const double2*>(Pc + c * Rp + kFNB);
            const double2 i01 = pc[ib >> 1], i23 = pc[(ib >> 1) + 1];
            const double2 l01 = pc[lb >> 1], l23 = pc[(lb >> 1) + 1];
            const double vi[4] = {i01.x, i01.y, i23.x, i23.y};
            const double vl[4] = {l01.x, l01.y, l23.x, l23.y};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) ac[a][b] = fma(vi[a], vl[b], ac[a][b]);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int l = lb + b;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int i = ib + a;
                if (l < w1 && i < R1 && i >= l) Pn[l * Rp1 + off1 + i] -= ac[a][b];
            }
        }
    }
}

// forward solve folded in: y of panel p's rows (one wave), then the rows below (bv, LDS)
__device__ void rhs_panel(int p, const Tiles& T, const double* P, double* bv) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PanelFrame f(T, p);
    const int j0 = f.j0, w = f.w, R = f.R, off = f.off, Rp = f.Rp;
    if (wave == 0) {
        double bl = lane < w ? bv[j0 + lane] : 0.0;
        for (int c = 0; c < w; ++c) {
            const double yc = __shfl(bl, c, 64) / P[c * Rp + off + c];
            if (lane == c) bl = yc;
            else if (lane > c && lane < w) bl = fma(-P[c * Rp + off + lane], yc, bl);
        }
        if (lane < w) bv[j0 + lane] = bl;
    }
    __syncthreads();
    for (int i = w + tid; i < R; i += kFT) {
        double sacc = 0.0;
        for (int c = 0; c < w; ++c) sacc = fma(P[c * Rp + off + i], bv[j0 + c], sacc);
        bv[j0 + i] -= sacc;
    }
    __syncthreads();
}

// A front of more than kSmall rows is factored by a TEAM of G workgroups (G consecutive tickets).
// Its columns are cut into tiles of kFNB: pivot tiles [kFNB t, min(kFNB t + kFNB, k3)), then update
// tiles from k3.  Member 0 runs the panel CHAIN and owns tile 0; tile t >= 1 belongs to helper
// 1 + (t - 1) mod (G - 1), which alone assembles it and applies the panels to it, except that the
// last panel before a pivot tile's own (panel t - 1) is applied by member 0:
//   assembly, per own tile, in LDS: H's blocks, then the children's update-matrix columns that land
//     in the tile (host-precomputed ranges), child by child, kFT * kPFL sc1 loads in flight;
//   chain (member 0): panel p is in LDS; it loads pivot tile p + 1 (handed off write-through by its
//     helper once panels 0..p-1 are in: flag tready[t]), applies panel p to it LDS to LDS, factors and
//     publishes it (write-through + panel flag) -- the chain never waits on a panel load or a flag it
//     could not have had a step earlier; with one LDS panel buffer (db == 0, very tall fronts) the
//     step goes through the front instead;
//   helpers: for p = 0, 1, ..: wait for panel p, load it, first bring pivot tile p + 2 up to date and
//     hand it off, then apply panel p to their other tiles;
//   the owner of the last tile (a helper that loads every panel) carries the right-hand side
//   (forward solve folded in, as in small_front);
//   at the end every member republishes its update tiles write-through and adds 1 to the parent's
//   counter (which waits for the sum of its children's team sizes).
__device__ __forceinline__ int tile_owner(int t, int G) { return t == 0 || G == 1 ? 0 : 1 + (t - 1) % (G - 1); }

__device__ __forceinline__ void large_front(int s, int mem, const SnDev& S, int32_t* sync, int32_t* pflag,
                            int32_t* tready, int32_t* status,
                            const SnDev* __restrict__ sns, const OEnt* __restrict__ omap,
                            const int32_t* __restrict__ relmap, const int32_t* __restrict__ child_list,
                            const FTask* __restrict__ ftasks, const FChild* __restrict__ fchild,
                            const double* __restrict__ hb, const double* __restrict__ g,
                            const int32_t* __restrict__ perm, double* fronts, double* __restrict__ ysol,
                            double* acc, double* sm, int db) {
    const int tid = threadIdx.x;
    const int k3 = 3 * S.k, r3 = 3 * S.r, m3 = k3 + r3, G = S.G;
    double* F = fronts + S.front_off;
    Tiles T{k3, m3, (k3 + kFNB - 1) / kFNB, 0};
    T.nt = T.np + (r3 + kFNB - 1) / kFNB;
    int32_t* trdy = tready + S.ftask;
    const bool has_b = mem == tile_owner(T.nt - 1, G);   // the right-hand side: a helper that sees every panel
    const int t_first = mem, t_step = mem == 0 ? T.nt : G - 1;   // own tiles: t_first, += t_step
    double* bv = sm;                               // [m3] right-hand side (member 0)
    double* scr = bv + ((m3 + 1) & ~1);            // POTRF / TRSM scratch
    double* PA = scr + kFScr;                      // tile under assembly / panel buffers
    double* PB = db ? PA + (size_t)kFNB * fused_rp(m3, 3) : PA;
    if (has_b)
        for (int t = tid; t < m3; t += kFT) bv[t] = t < k3 ? -g[3 * perm[S.c0 + t / 3] + t % 3] : 0.0;
    // ---- assembly of the own tiles in LDS (the first one's H blocks before the wait)
    bool waited = S.need == 0;
    for (int t = t_first; t < T.nt; t += t_step) {
        const FTask tk = ftasks[S.ftask + t];
        const int cs = T.c0(t), nc = T.c1(t) - cs;
        double* Tl = PA;                           // [nc][m3] column-major
        for (int e = tid; e < nc * m3; e += kFT) Tl[e] = 0.0;
        __syncthreads();
        for (int q = tid; q < (tk.om_e - tk.om_b) * 9; q += kFT) {
            const OEnt o = omap[tk.om_b + q / 9];
            const int ii = (q % 9) / 3, jj = q % 3;
            const int row = 3 * o.a + ii, col = 3 * o.b + jj;
            if (col < cs || col >= cs + nc || row < col) continue;
            const double* B = hb + 9 * (int64_t)o.u;
            Tl[(col - cs) * m3 + row] = o.tr ? B[3 * jj + ii] : B[3 * ii + jj];
        }
        if (!waited) {
            if (tid == 0) wait_geq_sc1(sync + s, S.need, status);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            waited = true;
            FT_MARK(s, 1);
        }
        for (int cq = 0; cq < tk.ch_cnt; ++cq) {
            __syncthreads();
            const FChild C = fchild[tk.ch_off + cq];
            const int n = 3 * C.r, m3c = 3 * (C.k + C.r), k3c = 3 * C.k, nj = C.jb - C.ja;
            // the child's update matrix: column j of it, rows i >= j, is front element
            // (k3c + j) m3c + k3c + i -- 16-B sc1 loads of the aligned pairs over each column
            const auto rs = front_rsrc(fronts + C.front_off, m3c);
            const int32_t* rm = relmap + C.rows_off;
            const int npc = (n + 2) >> 1, tot = nj * npc;
            for (int e0 = 0; e0 < tot; e0 += kFT * kPFL) {
                double2 v[kPFL];
                int d0[kPFL], d1[kPFL];
#pragma unroll
                for (int q = 0; q < kPFL; ++q) {
                    const int e = e0 + tid + kFT * q;
                    const int jj = e / npc, k = e - jj * npc, j = C.ja + jj;
                    const uint32_t a = (uint32_t)((k3c + j) * m3c + k3c);
                    const int i0 = 2 * k - (int)(a & 1u);
                    d0[q] = -1;
                    d1[q] = -1;
                    v[q] = make_double2(0.0, 0.0);
                    if (e < tot && i0 + 1 >= j && i0 < n) {
                        v[q] = ld2_sc1(rs, (a & ~1u) + 2u * k);
                        const int cj = (3 * rm[j / 3] + j % 3 - cs) * m3;
                        if (i0 >= j) d0[q] = cj + 3 * rm[i0 / 3] + i0 % 3;
                        if (i0 + 1 < n) d1[q] = cj + 3 * rm[(i0 + 1) / 3] + (i0 + 1) % 3;
                    }
                }
#pragma unroll
                for (int q = 0; q < kPFL; ++q) {
                    if (d0[q] >= 0) Tl[d0[q]] += v[q].x;
                    if (d1[q] >= 0) Tl[d1[q]] += v[q].y;
                }
            }
        }
        __syncthreads();
        if (t == 0 && mem == 0 && db) {
            // the chain's first panel straight from the assembled tile: LDS to LDS into the panel
            // frame of PB (zeros above the diagonal, as load_panel), no round trip through the front
            const int off = (4 - (nc & 3)) & 3, Rp = fused_rp(m3, off);
            for (int e = tid; e < nc * m3; e += kFT) {
                const int c = e / m3, i = e - c * m3;
                PB[c * Rp + off + i] = i >= c ? Tl[e] : 0.0;
            }
            __syncthreads();
            continue;
        }
        const bool handoff = t == 1 && mem != 0;   // pivot tile 1 goes to the chain as assembled
        for (int e = tid; e < nc * m3; e += kFT) {
            const int col = cs + e / m3, row = e % m3;
            if (row >= col) {
                if (handoff) st_agent(F + (uint32_t)(col * m3 + row), Tl[e]);
                else F[(uint32_t)(col * m3 + row)] = Tl[e];
            }
        }
        if (handoff) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (handoff && tid == 0) __hip_atomic_store(trdy + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!waited) {   // a helper without tiles (G > nt cannot happen; kept for safety)
        if (tid == 0) wait_geq_sc1(sync + s, S.need, status);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (has_b) {   // the children's pending row updates, child order
        for (int ci = 0; ci < S.nchild; ++ci) {
            const SnDev C = sns[child_list[S.child_off + ci]];
            const int32_t* rm = relmap + C.rows_off;
            for (int t = tid; t < 3 * C.r; t += kFT) bv[3 * rm[t / 3] + t % 3] -= ld_agent(acc + C.acc_off + t);
            __syncthreads();
        }
    }
    FT_MARK(s, 2);

    bool bad = false;
    if (mem == 0) {
        // ---- the panel chain
        double* cur = db ? PB : PA;   // db: panel 0 is in PB already (the assembly's relayout)
        if (tid < kFNB / 3) reinterpret_cast<int*>(scr + kFNB * kFNB + 8 * (kFNB / 3))[tid] = 0;   // POTRF step epochs
        if (!db) load_panel<false>(0, T, F, cur);   // tile 0: assembled by this workgroup
        __syncthreads();
        factor_lds(0, s, T, cur, scr, bad);
        publish_panel(0, s, T, F, cur, pflag);
        for (int p = 0; p < T.np; ++p) {
            double* nxt = cur == PA ? PB : PA;
            if (has_b && !db) rhs_panel(p, T, cur, bv);
            if (p + 1 < T.np) {
                const int t = p + 1;
                PN_MARK(s, t, 0);
                if (tile_owner(t, G) != 0) {
                    if (tid == 0) wait_geq_sc1(trdy + t, 1, status);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                }
                if (db) {
                    load_panel<true>(t, T, F, nxt);
                    __syncthreads();
                    PN_MARK(s, t, 1);
                    update_next_lds(p, T, cur, nxt);
                } else {   // through the front: sc1 reads of the handed-off tile, then reload
                    PN_MARK(s, t, 1);
                    update_tile<true, true>(t, p, T, F, cur);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    load_panel<true>(t, T, F, nxt);
                }
                __syncthreads();
                PN_MARK(s, t, 2);
                factor_lds(t, s, T, nxt, scr, bad);
                publish_panel(t, s, T, F, nxt, pflag);
            }
            if (has_b && db) rhs_panel(p, T, cur, bv);
            cur = nxt;
        }
    } else {
        // ---- helpers: apply each panel to the own tiles right of it (pivot tile p + 1 excepted)
        double* P = PA;
        for (int p = 0; p < T.np; ++p) {
            bool need = false;
            for (int t = t_first; t < T.nt; t += t_step) need |= t > p && !(t == p + 1 && t < T.np);
            if (!need && !has_b) break;
            if (tid == 0) wait_geq_sc1(pflag + s, p + 1, status);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            load_panel<true>(p, T, F, P);
            __syncthreads();
            const int tc = p + 2;   // the chain's next-but-one tile first, handed off when done
            const bool mine = tc < T.np && tile_owner(tc, G) == mem;
            if (mine) {
                update_tile<true>(tc, p, T, F, P);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(trdy + tc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // the last panel's update of an update tile is its final value: stored write-through for
            // the parent (no republishing pass after the chain)
            const bool fin = p == T.np - 1 && S.parent >= 0;
            for (int t = t_first; t < T.nt; t += t_step)
                if (t > p && !(t == p + 1 && t < T.np) && !(mine && t == tc)) {
                    if (fin) update_tile<true>(t, p, T, F, P);
                    else update_tile<false>(t, p, T, F, P);
                }
            __syncthreads();
            if (has_b) rhs_panel(p, T, P, bv);
        }
    }
    if (bad && (tid & 63) == 0) atomicExch(status, 1);
    // ---- out: member 0 (or the right-hand side's owner): y and the pending updates
    if (has_b) {
        for (int t = tid; t < k3; t += kFT) ysol[3 * (int64_t)S.c0 + t] = bv[t];
        if (S.parent >= 0)
            for (int t = tid; t < r3; t += kFT) st_agent(acc + S.acc_off + t, -bv[k3 + t]);
    }
    FT_MARK(s, 3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (mem == 0) FT_MARK(s, 4);
    if (tid == 0 && S.parent >= 0)
        __hip_atomic_fetch_add(sync + S.parent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kFT, 2) void chol_factor_dag(const int32_t* __restrict__ order, int32_t* sync,
                                                       int32_t* status, const SnDev* __restrict__ sns,
                                                       const OEnt* __restrict__ omap,
                                                       const int32_t* __restrict__ relmap,
                                                       const int32_t* __restrict__ child_list,
                                                       const FTask* __restrict__ ftasks,
                                                       const FChild* __restrict__ fchild,
                                                       const double* __restrict__ hb, const double* __restrict__ g,
                                                       const int32_t* __restrict__ perm, double* fronts,
                                                       double* __restrict__ ysol, double* acc, int ns, int db,
                                                       const int32_t* gate, const uint8_t* __restrict__ keep) {
    extern __shared__ __attribute__((aligned(16))) double smem_f[];
    double* sm = smem_f + 2;   // smem_f[0]: the claimed ticket (no static LDS: keeps the base 16-B aligned)
    if (gate_off(gate, 1)) return;
    // issue priority over co-resident waves of other kernels (the batch covariance runs beside the
    // first factorization of a step, dpg_icp_batch_run): this kernel is a chain of dependent steps
    __builtin_amdgcn_s_setprio(2);
    const int code = claim_lds(order, sync, reinterpret_cast<int*>(smem_f));
    const int s = code >> 6, mem = code & 63;
    const SnDev S = sns[s];
    if (keep && keep[s]) {   // partial refactorization: the front keeps its factored values (and its
                             // update matrix, which the parent reads as from a finished member)
        if (threadIdx.x == 0 && S.parent >= 0)
            __hip_atomic_fetch_add(sync + 1 + S.parent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (mem == 0) FT_MARK(s, 0);
    if (S.G == 1 && 3 * (S.k + S.r) <= kSmall && S.nchild <= kMaxCh)
        small_front(s, S, sync + 1, status, sns, omap, relmap, child_list, hb, g, perm, fronts, ysol, acc, sm);
    else
        large_front(s, mem, S, sync + 1, sync + 1 + ns, sync + 2 + 3 * ns, status, sns, omap, relmap, child_list,
                    ftasks, fchild, hb, g, perm, fronts, ysol, acc, sm, db);
}

// partial refactorization: the kept fronts (and their pending forward-solve updates) the new layout
// moved, as runs {src, dst, doubles, buffer} (one run per blockIdx.y; buffer 0: fronts, 1: the
// pending updates), through a scratch buffer (gather, then scatter: old and new places overlap)
__global__ __launch_bounds__(256) void chol_copy_runs(const double* __restrict__ src0, const double* __restrict__ src1,
                                                      double* __restrict__ dst0, double* __restrict__ dst1,
                                                      const int64_t* __restrict__ runs) {
    const int64_t* r = runs + 4 * blockIdx.y;
    const int64_t s0 = r[0], d0 = r[1], n = r[2];
    const double* src = r[3] ? src1 : src0;
    double* dst = r[3] ? dst1 : dst0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[d0 + i] = src[s0 + i];
}

}  // namespace

void dpg_chol::launch_factor(CholDev* c, hipStream_t st, const double* hb, const int32_t* gate, const uint8_t* keep) {
    const CholPlan& P = c->plan;
    hipLaunchKernelGGL(chol_factor_dag, dim3((unsigned)P.n_tickets), dim3(kFT), P.lds_fused, st, c->order_fac, sync_forward(c),
                       c->status.p, c->sns, c->omap, c->relmap, c->child_list, c->ftasks, c->fchild, hb, hb + 9 * P.nnzb_upper,
                       c->perm, c->fronts.p, c->ysol.p, c->acc.p, c->sym.ns, P.fused_db ? 1 : 0, gate, keep);
}

void dpg_chol::launch_copy_runs(CholDev* c, hipStream_t st, const int64_t* gather, const int64_t* scatter, int64_t nruns,
                                int64_t max_run) {
    if (nruns == 0) return;
    const dim3 grid((unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (max_run + 2047) / 2048)), (unsigned)nruns);
    hipLaunchKernelGGL(chol_copy_runs, grid, dim3(256), 0, st, c->fronts.p, c->acc.p, c->scratch.p, c->scratch.p, gather);
    hipLaunchKernelGGL(chol_copy_runs, grid, dim3(256), 0, st, c->scratch.p, c->scratch.p, c->fronts.p, c->acc.p, scatter);
}
